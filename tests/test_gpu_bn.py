"""-m gpu: every BatchNorm leaf of csrc/elementwise.hip through the strict comparator of tests/strict_bn.py: float64
references from exactly the buffers each stage receives, derived per-element limits (proved on the CPU by
tests/test_strict_bn_cpu.py).

Both paths, on every case:
  accumulator    bn_stats_acc -> bn_act_fwd_train (and bn_finalize_acc) -> bn_act_bwd_train; acc_f and acc_b are read after
                 the calls, every stage is compared from the accumulator and the coefficients the kernel published.  Float
                 atomics: not asserted to repeat.
  deterministic  bn_train_stats -> bn_act_fwd -> bn_act_bwd / bn_act_bwd_eval, channel_sum, bn_eval_coeffs; the partial rows
                 are not exposed, so the sums' limit enters the coefficients' as an input error.  Every call runs twice and
                 must repeat bit for bit.
out= as a channel slice of a wider buffer must leave the neighbouring channels bit-identical (bn_act_fwd, bn_act_fwd_train).
The module prints the largest share of the noise budget per family and the `offset` headroom figures when it finishes."""
import pytest
import torch

import strict_bn as sb
import strict_compare as sc
from test_gpu_kernels import DEV, dev, nhwc, ops

pytestmark = pytest.mark.gpu
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]
# n, c, h, w, pad (the tensors are channel slices pad / 2 channels into a buffer of c + pad channels), residual
SHAPES = [
    (3, 6, 11, 13, 0, True),        # one element per lane, 6 lanes per row, threads 252..255 idle
    (3, 24, 11, 13, 16, False),     # 8 channels into a wider buffer: 16-byte packets for every type
    (3, 24, 11, 13, 8, False),      # 4 channels in: packets for fp32 only, 16-bit one element per lane
    (3, 24, 11, 13, 4, False),      # 2 channels in: one element per lane for every type
    (3, 264, 11, 13, 0, True),      # 16-lane rows, partly filled last channel group, main loop and tail both run
    (3, 264, 11, 13, 4, False),     # one element per lane with 264 > 256 lanes: two blockIdx.y groups (17 in the narrow plan)
    (2, 2056, 3, 5, 0, False),      # 257 packets of 8: the second blockIdx.y group holds one channel group
    (1, 8, 1, 3, 0, False),         # fewer pixels than rows per workgroup
    (1, 16, 1, 1, 0, False),        # one pixel: the unbiased variance takes the biased one
]
LARGE = (2, 264, 110, 100, 0, False)   # 22 000 pixels: more than one main-loop iteration per thread
HEADROOM = {}                          # (dtype, path) -> [max relative error of invstd, max dgamma error / max |dgamma|, / (U mass)]


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    yield
    print("\n" + sc.report())
    for (dtype, path), v in sorted(HEADROOM.items(), key=str):
        print(f"[strict_bn] offset, {str(dtype)[6:]:8s} {path:13s}: invstd relative error {v[0]:.3e}; dgamma error {v[1]:.3e} of max |dgamma|, "
              f"{v[2]:.2f} x 2^-24 of its mass invstd sum |dz y|   (against float64 from the inputs)")


def headroom(case, path, invstd, dgamma):
    if case.count < 100 or case.pdt != F32:                    # a handful of pixels: dgamma is all cancellation; a 16-bit
        return                                                 # dgamma: the figure would be that type's rounding
    t = sb.truth(case)
    err = (sb.d64(dgamma) - t["dgamma"]).abs()
    v = [float(((sb.d64(invstd) - t["invstd"]).abs() / t["invstd"]).max()), float(err.max() / t["dgamma"].abs().max()),
         float((err / (sb.U24 * t["dgamma_mass"])).max())]
    h = HEADROOM.setdefault((case.dtype, path), [0.0, 0.0, 0.0])
    h[:] = [max(a, b) for a, b in zip(h, v)]


def in_slice(o, n, c, h, w, dtype):
    """-> (buffer of c + 16 channels holding a seeded bit pattern, its copy, the slice 8 channels in)"""
    g = torch.Generator().manual_seed(7)
    buf = o.new_nhwc(n, c + 16, h, w, dtype, DEV)
    buf.copy_(torch.randn(n, c + 16, h, w, generator=g).to(dtype))
    return buf, buf.clone(), buf[:, 8:8 + c]


def neighbours_untouched(buf, before, c):
    return torch.equal(buf[:, :8], before[:, :8]) and torch.equal(buf[:, 8 + c:], before[:, 8 + c:])


def run_both_paths(case, pad):
    o = ops()
    n, c, h, w = case.shape
    y, dout, res = dev(nhwc(case.y, pad)), dev(nhwc(case.dout, pad)), None if case.res is None else dev(nhwc(case.res))
    gamma, beta = case.gamma.to(DEV), case.beta.to(DEV)
    mom, eps, act = case.momentum, case.eps, case.act

    # ---- accumulator path
    acc_f, acc_b = o.bn_acc_new(c, DEV), o.bn_acc_new(c, DEV)
    o.bn_stats_acc(y, acc_f)
    rm, rv = case.rmean.to(DEV), case.rvar.to(DEV)
    out, mean, invstd, scale, shift = o.bn_act_fwd_train(y, acc_f, gamma, beta, rm, rv, mom, eps, act, res)
    dy, dgamma, dbeta = o.bn_act_bwd_train(dout, y, scale, shift, mean, invstd, gamma, act, acc_b)
    sb.verify_accumulator_path(case, {"acc_f": acc_f, "acc_b": acc_b, "mean": mean, "invstd": invstd, "scale": scale, "shift": shift,
                                      "rmean": rm, "rvar": rv, "out": out, "dy": dy, "dgamma": dgamma, "dbeta": dbeta})
    if case.cls == "offset":
        headroom(case, "accumulator", invstd, dgamma)
    rm2, rv2 = case.rmean.to(DEV), case.rvar.to(DEV)
    fin = o.bn_finalize_acc(acc_f, case.count, gamma, beta, rm2, rv2, mom, eps)
    sb.check_coef(case, fin, *sb.fold(acc_f, c), rmean=rm2, rvar=rv2, what="finalize_acc")
    buf, before, view = in_slice(o, n, c, h, w, case.dtype)
    out2 = o.bn_act_fwd_train(y, acc_f, gamma, beta, case.rmean.to(DEV), case.rvar.to(DEV), mom, eps, act, res, out=view)[0]
    assert out2.data_ptr() == view.data_ptr() and neighbours_untouched(buf, before, c), f"{case.what}: bn_act_fwd_train out= slice"
    sb.check_out(case, view, scale, shift, case.res, mult=2.0, what="acc out= slice")

    # ---- deterministic path, twice
    def det():
        rm, rv = case.rmean.to(DEV), case.rvar.to(DEV)
        mean, invstd, scale, shift = o.bn_train_stats(y, gamma, beta, rm, rv, mom, eps)
        r = {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "rmean": rm, "rvar": rv,
             "out": o.bn_act_fwd(y, scale, shift, act, res)}
        r["dy"], r["dgamma"], r["dbeta"] = o.bn_act_bwd(dout, y, scale, shift, mean, invstd, gamma, act)
        r["dy_eval"] = o.bn_act_bwd_eval(dout, y, scale, shift, act)
        r["csum"] = o.channel_sum(dout)
        r["eval_scale"], r["eval_shift"] = o.bn_eval_coeffs(gamma, beta, rm, rv, eps)
        return r
    r, again = det(), det()
    for k in r:
        assert torch.equal(r[k], again[k]), f"{case.what}: {k} of the deterministic path does not repeat bit for bit"
    sb.verify_deterministic_path(case, r)
    if case.cls == "offset":
        headroom(case, "deterministic", r["invstd"], r["dgamma"])
    buf, before, view = in_slice(o, n, c, h, w, case.dtype)
    o.bn_act_fwd(y, r["scale"], r["shift"], act, res, out=view)
    assert neighbours_untouched(buf, before, c), f"{case.what}: bn_act_fwd out= slice"
    assert torch.equal(view, r["out"]), f"{case.what}: bn_act_fwd into a slice differs from the same call into a fresh tensor"


@pytest.mark.parametrize("cls", sb.CLASSES)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:4])) + f"+{s[4]}")
def test_bn_leaves_within_derived_limits(shape, dtype, act, cls):
    n, c, h, w, pad, with_res = shape
    run_both_paths(sb.Case(cls, n, c, h, w, dtype, act, with_res), pad)


@pytest.mark.parametrize("cls", ["plain", "offset"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_leaves_within_derived_limits_at_22000_pixels(dtype, cls):
    n, c, h, w, pad, with_res = LARGE
    run_both_paths(sb.Case(cls, n, c, h, w, dtype, 1, with_res), pad)


@pytest.mark.parametrize("bdt", [BF, HF], ids=["buf-bf16", "buf-f16"])
@pytest.mark.parametrize("pdt", [BF, HF], ids=["par-bf16", "par-f16"])
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
def test_bn_16_bit_parameters_and_buffers(dtype, pdt, bdt):
    """gamma / beta and the running statistics in the low-precision types of the FSDP mixed-precision contract: dgamma and
    dbeta come back in the parameter's type within 1/2 ulp of it, the running statistics within their limit and 1/2 ulp of
    the buffer's type (strict_bn.check_coef / check_bwd assert the types)"""
    for cls in ("plain", "offset"):
        run_both_paths(sb.Case(cls, 3, 24, 11, 13, dtype, 1, False, pdt=pdt, bdt=bdt), 0)


def test_bn_mixed_parameter_dtypes_raise():
    o = ops()
    case = sb.Case("plain", 3, 24, 11, 13, BF, 1)
    y = dev(nhwc(case.y))
    gamma, beta, rm, rv = case.gamma.to(DEV), case.beta.to(DEV), case.rmean.to(DEV), case.rvar.to(DEV)
    acc = o.bn_acc_new(24, DEV)
    o.bn_stats_acc(y, acc)
    for g, b, m, v in ((gamma.to(BF), beta.to(HF), rm, rv), (gamma, beta.to(BF), rm, rv), (gamma, beta, rm.to(BF), rv.to(HF)),
                       (gamma, beta, rm, rv.to(HF))):
        with pytest.raises(RuntimeError):
            o.bn_finalize_acc(acc, case.count, g, b, m, v, 0.03, 1e-3)
        with pytest.raises(RuntimeError):
            o.bn_act_fwd_train(y, acc, g, b, m, v, 0.03, 1e-3, 1)
        with pytest.raises(RuntimeError):
            o.bn_train_stats(y, g, b, m, v, 0.03, 1e-3)
        with pytest.raises(RuntimeError):
            o.bn_eval_coeffs(g, b, m, v, 1e-3)
