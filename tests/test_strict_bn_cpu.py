"""CPU tests of tests/strict_bn.py: what proves, without a GPU, that the derived per-element BatchNorm limits pass the
kernels' arithmetic and fail arithmetic that is subtly wrong.

The stand-in is fp32 torch code with the kernels' rounding points (csrc/elementwise.hip): fp32 sums into 8 replicas, the
fold and bn_fwd_coef / bn_bwd_coef in double with their (float) casts, z = y scale + shift, silu through 1 / (1 + exp(-z)),
dz = dout act'(z), dy = A dz + B y + D, one rounding to the tensor's type, parameters and running statistics in their own
types.  Two summation orders:
  order 0   strided thread partials of at most four pixels each, added pairwise (a tree) into the 8 replicas
  order 1   pixel order: 64 consecutive pixels are added one after another, the chunk sums one after another into replica
            (chunk index mod 8): at 22 000 pixels a chain of 64 and one of 43, as the workgroups' float atomics form
Both must have NOTHING outside any limit on every shape of tests/test_gpu_bn.py, in fp32 / bf16 / f16, on the four input
classes and both activations, through the stage-wise checks (accumulator path) AND the composed ones (deterministic
path); every mutant of MUTANTS must raise StrictMismatch, in the family named beside it.

Recorded maxima of the stand-ins, largest share of the noise budget used ((|got - ref| - 1/2 ulp) / noise, limit 1; the
module prints the table when it finishes, run with -s): see STAND_IN_MAXIMA below."""
import contextlib
import math
import re

import pytest
import torch

import strict_bn as sb
import strict_compare as sc

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]
# n, c, h, w, residual: the shapes of tests/test_gpu_bn.py (a channel slice of a wider buffer is the same arithmetic)
SHAPES = [(3, 6, 11, 13, True), (3, 24, 11, 13, False), (3, 264, 11, 13, True), (2, 2056, 3, 5, False), (1, 8, 1, 3, False),
          (1, 16, 1, 1, False)]
LARGE = (2, 264, 110, 100, False)
CHUNK = 64                         # pixels of one serial chain in the pixel-order stand-in
GROUP = 256                        # channels of one blockIdx.y group at one element per lane
STAND_IN_MAXIMA = """sum y 0.28, sum y^2 0.30 (4.8 x 2^-24 of the mass), sum dz 0.17, sum dz y 0.19, coefficients 0.96,
out 0.57, dgamma 0.12, dbeta 0.17, dy 0.64.  (What the chain lengths are for: ONE chain over 2750 squares of bf16 values near 6
-- all on a grid of 2^-10, so that every rounding is a tie and round-to-even drops each -- lands 250 x 2^-24 of the mass low.
The kernels form no such chain: a thread adds a few pixels, a workgroup its rows, a replica 43 workgroups at 22 000 pixels.)"""


@pytest.fixture(autouse=True, scope="module")
def _threads_and_report():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    yield
    print("\n" + sc.report())


# ------------------------------------------------------------------------------------------ the stand-in (fp32)
def rows(t):
    """(N, C, H, W) -> (pixels, C) fp32, pixel-major as the kernels walk NHWC memory"""
    return t.float().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def replicas(x, order, mut=None, w=1):
    """fp32 sums of the pixel rows x (P, C) into 8 replicas (8, C)"""
    if mut == "last_pixel_row_missing":
        x = x[:-w]
    if mut == "tail_rows_skipped":                           # only whole RS_ROWS x step (2 x 32) blocks of pixels
        x = x[:x.shape[0] - x.shape[0] % 64]
    p, c = x.shape
    if order == 0:
        lanes = 8 * 2 ** max(2, math.ceil(math.log2(max(1.0, p / 32))))
        steps = math.ceil(p / lanes)
        v = torch.cat([x, torch.zeros(steps * lanes - p, c)]).view(steps, lanes, c)
        acc = torch.zeros(lanes, c)
        for t in range(steps):                                # thread partials, at most four pixels each
            acc = acc + v[t]
        while acc.shape[0] > 8:                               # the tree
            acc = acc[0::2] + acc[1::2]
        return acc
    chunks = 8 * math.ceil(p / (8 * CHUNK))
    v = torch.cat([x, torch.zeros(chunks * CHUNK - p, c)]).view(chunks, CHUNK, c)
    part = torch.zeros(chunks, c)
    for t in range(CHUNK):                                    # 64 consecutive pixels one after another
        part = part + v[:, t]
    acc = torch.zeros(8, c)
    for t in range(chunks // 8):                              # chunk k into replica k % 8, in chunk order (the atomics)
        acc = acc + part[8 * t:8 * t + 8]
    return acc


def folded(acc, c, mut):
    a = acc.view(8, 2, c).double()
    a = a[:7] if mut == "seven_of_eight_replicas" else a
    return a.sum(0)


def act_grad(z, act, mut=None):
    if not act:
        return torch.ones_like(z)
    s = 1.0 / (1.0 + torch.exp(-z))
    return s if mut == "act_grad_without_z_term" else s * (1.0 + z * (1.0 - s))


def bc(v):
    return v.view(1, -1, 1, 1)


def stale_group(v, mut):
    """the channels of the second blockIdx.y group take the first group's constants"""
    if mut == "second_group_stale_coefficients" and v.numel() > GROUP:
        v = v.clone()
        v[GROUP:] = v[:v.numel() - GROUP]
    return v


def stand_in(case, order=0, mut=None):
    """-> dict of everything the two GPU paths leave behind (strict_bn.verify_*_path)"""
    n, c, h, w = case.shape
    cnt = case.count
    low = BF if case.dtype == F32 else case.dtype
    y, dout = case.y.float(), case.dout.float()
    yr = rows(case.y)
    acc_f = torch.stack([replicas(yr, order, mut, w), replicas(yr * yr, order, mut, w)], 1).reshape(-1)
    s, q = folded(acc_f, c, mut)
    # bn_fwd_coef / bn_fwd_publish
    m = s / cnt
    var = (q / cnt - m * m).clamp_min(0.0)
    invstd = ((var + sb.f32_of(case.eps)) ** -0.5).float()
    mean = m.float()
    gamma, beta = case.gamma.float(), case.beta.float()
    scale = gamma * invstd
    shift = beta - (mean.to(low).float() if mut == "mean_rounded_to_16_bits" else mean) * scale
    unbiased = (var * (cnt / (cnt - 1.0)) if cnt > 1 and mut != "running_var_biased" else var).float()
    mom = torch.tensor(case.momentum, dtype=F32)
    rmean = ((1.0 - mom) * case.rmean.float() + mom * mean).to(case.bdt)
    rvar = ((1.0 - mom) * case.rvar.float() + mom * unbiased).to(case.bdt)
    # bn_act_fwd_rows
    sc_, sh_ = stale_group(scale, mut), stale_group(shift, mut)
    z = y * bc(sc_) + bc(sh_)
    res = None if case.res is None else case.res.float()
    if mut == "residual_before_activation" and res is not None:
        z, res = z + res, None
    out = z * (1.0 / (1.0 + torch.exp(-z))) if case.act else z
    out = (out if res is None else out + res).to(case.dtype)
    # backward reduction
    z = y * bc(scale) + bc(shift)
    dz = dout * act_grad(z, case.act, mut)
    acc_b = torch.stack([replicas(rows(dz), order, mut, w), replicas(rows(dz * y), order, mut, w)], 1).reshape(-1)
    s, q = folded(acc_b, c, mut)
    # bn_bwd_coef
    inv, mu = invstd.double(), mean.double()
    cb = cnt + w if mut == "count_plus_one_image_row" else cnt
    dg = inv * (q - mu * s)
    k0, c1, c2 = gamma.double() * inv, s / cb, dg / cb
    a, b = k0.float(), (0.0 * k0 if mut == "dy_without_dgamma_term" else -k0 * c2 * inv).float()
    d = ((0.0 * k0 if mut == "dy_without_mean_term" else -k0 * c1) +
         (0.0 * k0 if mut == "dy_without_dgamma_term" else k0 * c2 * mu * inv)).float()
    dgamma = ((inv * q) if mut == "dgamma_not_centred" else dg).float().to(case.pdt)
    dy = (bc(a) * dz + bc(b) * y + bc(d)).to(case.dtype)
    dy_eval = (bc(scale) * dz).to(case.dtype)
    ev = gamma / torch.sqrt(rvar.float() + torch.tensor(case.eps, dtype=F32))
    return {"acc_f": acc_f, "acc_b": acc_b, "mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "rmean": rmean,
            "rvar": rvar, "out": out, "dy": dy, "dgamma": dgamma, "dbeta": s.float().to(case.pdt), "dy_eval": dy_eval,
            "csum": folded(torch.stack([replicas(rows(case.dout), order), torch.zeros(8, c)], 1).reshape(-1), c, None)[0].float(),
            "eval_scale": ev, "eval_shift": beta - rmean.float() * ev}


def run(cls, shape, dtype, act, order=0, mut=None, pdt=F32, bdt=F32):
    n, c, h, w, with_res = shape
    case = sb.Case(cls, n, c, h, w, dtype, act, with_res, pdt, bdt)
    r = stand_in(case, order, mut)
    sb.verify_accumulator_path(case, r)
    sb.verify_deterministic_path(case, r)


# ------------------------------------------------------------------------------------------ the stand-ins pass
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
def test_stand_in_has_nothing_outside(shape, dtype):
    for cls in sb.CLASSES:
        for act in (0, 1):
            for order in (0, 1):
                run(cls, shape, dtype, act, order)


@pytest.mark.parametrize("cls", ["plain", "offset"])
def test_stand_in_has_nothing_outside_at_22000_pixels(cls):
    for order in (0, 1):
        run(cls, LARGE, BF, 1, order)


@pytest.mark.parametrize("pdt,bdt", [(BF, BF), (HF, HF), (BF, F32), (F32, HF)], ids=["bf16", "f16", "bf16-f32", "f32-f16"])
def test_stand_in_with_16_bit_parameters_and_buffers(pdt, bdt):
    for cls in sb.CLASSES:
        for dtype in (BF, HF):
            run(cls, SHAPES[1], dtype, 1, 0, pdt=pdt, bdt=bdt)


# ------------------------------------------------------------------------------------------ the mutants fail
# mutant -> the family whose limit catches it first (the checks run in the order of the data flow)
MUTANTS = {"dy_without_mean_term": "bn_dy", "dy_without_dgamma_term": "bn_dy", "count_plus_one_image_row": "bn_dy",
           "last_pixel_row_missing": "bn_sum", "tail_rows_skipped": "bn_sum", "seven_of_eight_replicas": "bn_coef",
           "dgamma_not_centred": "bn_dgamma", "running_var_biased": "bn_coef", "mean_rounded_to_16_bits": "bn_coef",
           "residual_before_activation": "bn_fwd", "act_grad_without_z_term": "bn_bwd_sum",
           "second_group_stale_coefficients": "bn_fwd"}
SILU_ONLY = ("residual_before_activation", "act_grad_without_z_term")
SMALL = [SHAPES[0], SHAPES[1], SHAPES[2]]


@contextlib.contextmanager
def wrong_on_purpose():
    """no guard 'nowhere wider than before' (1/2 ulp of a wild `got` is wide), and nothing recorded among the maxima"""
    saved = {k: list(v) for k, v in sc.OBSERVED.items()}
    sb.GUARD = False
    try:
        yield
    finally:
        sb.GUARD = True
        sc.OBSERVED.clear()
        sc.OBSERVED.update(saved)


def caught_by(cls, shape, dtype, act, mut):
    """the family that raised StrictMismatch, or None"""
    with wrong_on_purpose():
        try:
            run(cls, shape, dtype, act, 0, mut)
        except sb.StrictMismatch as ex:
            return re.search(r" \[(bn_\w+), c = ", str(ex)).group(1)
    return None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mut", list(MUTANTS))
def test_every_mutant_fails(mut, dtype):
    shapes = SMALL
    if mut == "residual_before_activation":
        shapes = [s for s in SMALL if s[4]]                  # needs a residual
    if mut == "second_group_stale_coefficients":
        shapes = [SHAPES[2]]                                  # needs more channels than one group holds
    # the biased variance differs from the unbiased one by mom var / (N - 1): at var = 1e-4 (`tiny`) that is 7e-9 on a
    # running variance near 1, below the spacing of fp32 there: asserted on the classes where a buffer can show it
    classes = [c for c in sb.CLASSES if not (mut == "running_var_biased" and c == "tiny")]
    for shape in shapes:
        for cls in classes:
            for act in ((1,) if mut in SILU_ONLY else (0, 1)):
                assert caught_by(cls, shape, dtype, act, mut) == MUTANTS[mut], (mut, cls, shape, act)
    assert caught_by(classes[0], shapes[0], dtype, 1, None) is None     # and the same call without the mutant passes


def test_biased_running_variance_fails_at_three_pixels():
    """N = 3: the unbiased factor is 1.5"""
    for dtype in DTYPES:
        assert caught_by("plain", SHAPES[4], dtype, 0, "running_var_biased") == "bn_coef"


# ------------------------------------------------------------------------------------------ the gap this closes
def old_check_passes(got, want, dtype, mult):
    """check() of tests/test_gpu_kernels.py: the largest error against a share of the reference's largest magnitude"""
    got, want = got.float(), want.float()
    return float((got - want).abs().max()) <= sb.OLD_TOL[dtype] * mult * max(float(want.abs().max()), 1e-6)


def _old_test_case(c, dtype):
    """the inputs of test_bn_act_train_fwd_bwd (3 x C x 11 x 13, mean 0.3, std 1.5), identity activation"""
    case = sb.Case("plain", 3, c, 11, 13, dtype, 0)

    def rnd(*shape, seed):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    case.y = (rnd(3, c, 11, 13, seed=30) * 1.5 + 0.3).to(dtype)
    case.dout = rnd(3, c, 11, 13, seed=36).to(dtype)
    case.gamma, case.beta = 1 + 0.1 * rnd(c, seed=32), 0.1 * rnd(c, seed=33)
    return case


def _strict_dy_fails(case, r):
    with wrong_on_purpose():
        try:
            sb.check_bwd(case, r["scale"], r["shift"], r["mean"], r["invstd"], r["dy"], r["dgamma"], r["dbeta"],
                         acc=sb.fold(r["acc_b"], case.shape[1]))
        except sb.StrictMismatch as ex:
            return " [bn_dy, " in str(ex)
    return False


def test_the_former_limit_passes_two_mutants_the_strict_limit_fails():
    """check(dy, dy_ref, dtype, mult=2): a pixel count off by one image row passes it in bf16 and f16 at every channel
    count of test_bn_act_train_fwd_bwd, a dy without its sum(dz) / count term passes it in bf16 at C = 16; the strict
    limit fails both."""
    for dtype in (BF, HF):
        for c in (16, 24, 96, 6):
            case = _old_test_case(c, dtype)
            want, r = stand_in(case)["dy"], stand_in(case, mut="count_plus_one_image_row")
            assert old_check_passes(r["dy"], want, dtype, 2.0), (dtype, c)
            assert _strict_dy_fails(case, r), (dtype, c)
    case = _old_test_case(16, BF)
    want, r = stand_in(case)["dy"], stand_in(case, mut="dy_without_mean_term")
    assert old_check_passes(r["dy"], want, BF, 2.0)
    assert _strict_dy_fails(case, r)
    assert not _strict_dy_fails(case, stand_in(case))


# ------------------------------------------------------------------------------------------ the failure report
def test_failure_histograms_name_the_channel_block_and_the_pixel_block():
    case = sb.Case("plain", 3, 24, 11, 13, BF, 1)
    r = stand_in(case)
    r["out"][1, 17, 2, 3:5] += 0.5                           # image 1, channel 17, pixels (2, 3) and (2, 4)
    with wrong_on_purpose(), pytest.raises(sb.StrictMismatch) as ei:
        sb.check_out(case, r["out"], r["scale"], r["shift"])
    h = ei.value.hist
    assert set(h["image"]) == {1} and set(h["channel_block"]) == {1} and set(h["pixel_block"]) == {(143 + 2 * 13 + 3) // 16}, h
    r["scale"][17] *= 1.0 + 2.0 ** -20                        # a per-channel vector: the channel block of the one channel
    with wrong_on_purpose(), pytest.raises(sb.StrictMismatch) as ei:
        sb.check_coef(case, [r[k] for k in ("mean", "invstd", "scale", "shift")], *sb.fold(r["acc_f"], 24))
    assert set(ei.value.hist["channel_block"]) == {1} and ei.value.count == 1
