"""-m gpu: exact NaN / infinity propagation of the kernels between the image and the logits -- the dense, stem and depthwise
convolutions with their data and weight gradients and fused inference epilogues, the BatchNorm passes and attention -- by the
rule of tests/strict_nonfinite.py (proved on CPU stand-ins by tests/test_strict_nonfinite_cpu.py; cases, poison positions and
dependency sets: tests/nonfinite_cases.py, float64 references on indicator tensors, never the kernel).

Every case runs one clean launch, one NaN-poisoned and one +-inf-poisoned launch (outside the dependency set the result is
bit-identical to the clean one, inside it every element is NaN / non-finite) and one launch with NaN in everything it may
not read: the channels of the wider buffers beside every slice, the destination of a non-accumulating form and -- by handing
src.hipops.ops an allocator whose torch.empty comes back NaN-filled -- every scratch buffer, stash and workspace.
Then the f16 store overflow cases (derived, no tolerance) and one captured fp16 training step of the model whose overflow
arises inside the forward.  The module prints strict_nonfinite.report() when it finishes."""
import contextlib
import os

import pytest
import torch

import nonfinite_cases as nc
import strict_attention as sa
import strict_bn as sb
import strict_compare as sc
import strict_nonfinite as sn
from nonfinite_cases import BF, F32, HF, N

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
KIND_FAMILY = {1: "gather", 2: "halo", 3: "ring", 4: "rows", 5: "patch", 0: "generic"}


def ops():
    from src.hipops import ops as o
    return o


def lib():
    from src.hipops import lib as l
    return l


def lib_dt(dtype):
    return {BF: lib().BF16, HF: lib().F16, F32: lib().F32}[dtype]


@pytest.fixture(autouse=True)
def _reset_tuning():
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    yield
    lib().call("yolo_conv_tune_set", 0, -1, -1, -1, -1, 0, 0, 0)
    lib().call("yolo_wgrad_tune_set", 0, 0, 0, 0)
    lib().call("yolo_wgrad_tune_pf", 0)
    lib().call("yolo_dw_tune_set", 0)


@pytest.fixture(autouse=True, scope="module")
def _print_report():
    yield
    print("\n" + sn.report())


# ------------------------------------------------------------------------------------------------- hostile surroundings
def _nan_fill(t):
    if t.is_floating_point():
        t.fill_(NAN)
    elif t.dtype == torch.uint8:
        t.fill_(255)                                     # bytes of all ones: NaN as fp32, bf16 and f16
    return t


class _NanTorch:
    """stands in for the `torch` name inside src.hipops.ops: every torch.empty / empty_like comes back NaN-filled"""

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **k):
        return _nan_fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return _nan_fill(torch.empty_like(*a, **k))


@contextlib.contextmanager
def surroundings(hostile):
    """hostile: every buffer src.hipops.ops allocates (destinations, partials, stashes, workspaces, coefficient vectors)
    starts as NaN.  Accumulators the API wants zeroed are zeroed after the allocation (ops.bn_acc_new), as always."""
    o = ops()
    if not hostile:
        yield
        return
    real = o.torch
    o.torch = _NanTorch()
    try:
        yield
    finally:
        o.torch = real


def place(t, ld=None, fill=3.0, off=None):
    """NCHW-shaped CPU tensor -> NHWC device tensor, a channel slice in the middle of a buffer of ld channels holding `fill`
    (off: its first channel; default: the middle, rounded down to 8 channels)"""
    o = ops()
    n, c, h, w = t.shape
    ld = c if ld is None else ld
    buf = o.new_nhwc(n, ld, h, w, t.dtype, DEV)
    buf.fill_(fill)
    off = ((ld - c) // 2) // 8 * 8 if off is None else off
    view = buf[:, off:off + c]
    view.copy_(t.to(DEV))
    return view, (buf, off, off + c)


def fold(acc, c):
    return acc.detach().cpu().view(-1, 2, c).sum(0)


def all_bad(t, kind):
    t = t.detach().cpu().double()
    return bool(torch.isnan(t).all()) if kind == "nan" else bool((~torch.isfinite(t)).all())


# ------------------------------------------------------------------------------------------------- dense convolution
def dense_fwd(case, T, x, wt, hostile=False, stats=None):
    o = ops()
    cin, cout, k, s = case["cin"], case["cout"], case["k"], case["s"]
    oh, ow = nc.out_hw(case["h"], case["w"], k, s)
    stats = case["stats"] if stats is None else stats
    wp = o.pack_weights(wt.float().to(DEV), k, s, 0, T)
    fill = NAN if hostile else 3.0
    with surroundings(hostile):
        xd, gx = place(x, cin + 32, fill)
        ybuf = o.new_nhwc(N, cout + 16, oh, ow, T, DEV).fill_(fill)
        acc = o.bn_acc_new(cout, DEV) if stats else None
        y = o.conv_fwd(xd, wp, None, cout, k, s, acc, out=ybuf[:, 8:8 + cout])
    return y, acc, [gx, (ybuf, 8, 8 + cout)]


def dense_dgrad(case, T, form, dy, wt, base, a2, hostile=False):
    o = ops()
    cin, cout, h, w, k, s = (case[key] for key in ("cin", "cout", "h", "w", "k", "s"))
    wb = o.pack_weights(wt.float().to(DEV), k, s, 1, T)
    fill = NAN if hostile else 3.0
    with surroundings(hostile):
        dyd, gdy = place(dy, cout + 16, fill)
        if form == "plain":
            return o.conv_dgrad(dyd, wb, cin, h, w, k, s), [gdy]
        dxv, gdx = place(base, cin + 32, fill)
        a2v, ga2 = place(a2, cin + 24, fill) if form == "acc2" else (None, None)
        o.conv_dgrad(dyd, wb, cin, h, w, k, s, acc_into=dxv, acc2=a2v)
    return dxv, [gdy, gdx] + ([ga2] if ga2 else [])


def dense_fused(case, T, act, with_res, x, wt, bias, res, hostile=False):
    o = ops()
    cin, cout, k, s = case["cin"], case["cout"], case["k"], case["s"]
    oh, ow = nc.out_hw(case["h"], case["w"], k, s)
    wp = o.pack_weights(wt.float().to(DEV), k, s, 0, T)
    fill = NAN if hostile else 3.0
    with surroundings(hostile):
        xd, gx = place(x, cin + 32, fill)
        resd, gr = place(res, cout + 24, fill) if with_res else (None, None)
        ybuf = o.new_nhwc(N, cout + 16, oh, ow, T, DEV).fill_(fill)
        y = o.conv_fwd_act(xd, wp, bias.to(DEV), cout, k, s, act, resd, out=ybuf[:, 8:8 + cout])
        assert y is not None, "no MFMA kernel took this shape"
    return y, [gx, (ybuf, 8, 8 + cout)] + ([gr] if gr else [])


def dense_wgrad(case, T, x, dy, hostile=False):
    o = ops()
    cin, cout, k, s = case["cin"], case["cout"], case["k"], case["s"]
    fill = NAN if hostile else 3.0
    with surroundings(hostile):                          # the partials buffer and dw itself come back NaN-filled
        xd, gx = place(x, cin + 32, fill)
        dyd, gdy = place(dy, cout + 8, fill)
        dw = o.conv_wgrad(xd, dyd, k, s, F32)
    return dw, [gx, gdy]


def check_wgrad(case, T, inp, p, d, family, what):
    """NaN / inf in a few x channels -> exactly dw[:, ci] for the taps that exist; in a few dy channels -> exactly dw[co]"""
    k, s = case["k"], case["s"]
    clean, _ = dense_wgrad(case, T, inp["x"], inp["dy"])
    bound = None
    if family in sn.EXEMPT:
        ref, mass = sc.wgrad_ref(inp["x"], inp["dy"], tuple(clean.shape), k, s)
        bound = lambda merged: sc.assert_close(merged, ref, mass, F32, what, family)
    for kind in sn.KINDS:
        got, _ = dense_wgrad(case, T, sn.poison(inp["x"], p["x_w"], kind), inp["dy"])
        sn.assert_propagates(clean, got, d["wgrad_x"], kind, f"{what} x {kind}", family, bound)
        got, _ = dense_wgrad(case, T, inp["x"], sn.poison(inp["dy"], p["dy_w"], kind))
        sn.assert_propagates(clean, got, d["wgrad_dy"], kind, f"{what} dy {kind}", family, bound)
    if family not in sn.EXEMPT:
        # edge pixels alone: the taps that pair the poisoned pixel only with an output pixel past the map are left out (an
        # empty sum or 0 x NaN, nonfinite_cases.positions()); everything else is decided by the pixel-exact reference
        exact = d["wgrad_x_edge"]
        keep = exact | ~exact.any(0).flatten(1).any(1).view(1, -1, 1, 1).expand_as(exact)
        got, _ = dense_wgrad(case, T, sn.poison(inp["x"], p["x_edge"], "nan"), inp["dy"])
        sn.assert_propagates(clean.cpu()[keep], got.cpu()[keep], exact[keep], "nan", f"{what} x at the edges", family)

        def run(hostile):
            dw, guards = dense_wgrad(case, T, inp["x"], inp["dy"], hostile)
            return {"dw": dw}, guards
        sn.assert_unmoved_by_surroundings(run, what, family)
    else:
        # the atomics paths add into a matrix they zero themselves: with NaN surroundings the result stays inside the bound
        dw, guards = dense_wgrad(case, T, inp["x"], inp["dy"], True)
        bound(dw.cpu())
        sn.assert_unmoved_by_surroundings(lambda hostile: ({}, guards if hostile else []), what, family)


@pytest.mark.parametrize("case", nc.DENSE, ids=[c["id"] for c in nc.DENSE])
def test_dense_conv_forward_data_gradient_and_fused_epilogue(case, monkeypatch):
    o = ops()
    monkeypatch.setattr(o, "ALGO", case["algo"])
    cin, cout, h, w, k, s = (case[key] for key in ("cin", "cout", "h", "w", "k", "s"))
    oh, ow = nc.out_hw(h, w, k, s)
    p, d = nc.dense_plan(case)
    for T in case["dtypes"]:
        lib().call("yolo_conv_tune_set", *case["tune"])
        q = lib().query
        if case["plan"] is not None:
            got = q("yolo_conv2d_plan", N, h, w, cin, oh, ow, cout, k, s, 0, 0, lib_dt(T))
            assert got == case["plan"], f"test does not reach the variant it is written for: plan {got}, wanted {case['plan']}"
        dplans = [q("yolo_conv2d_plan", N, h, w, cin, oh, ow, cout, k, s, 1, c, lib_dt(T)) for c in range(4 if s == 2 else 1)]
        if case.get("dplan"):
            assert all(g == case["dplan"] for g in dplans), dplans
        fam = case["family"]
        dfam = fam if fam in ("generic", "fp32") or case["algo"] else KIND_FAMILY[dplans[0] // 1000]
        inp = nc.dense_inputs(case, T)
        sn.require_nonzero(case["id"], w=inp["w"], x=inp["x"], dy=inp["dy"])
        what = f"{case['id']} {str(T)[6:]}"
        x, wt = inp["x"], inp["w"]

        # ---- forward, with the statistics epilogue where the family has one
        y0, acc0, _ = dense_fwd(case, T, x, wt)
        for kind in sn.KINDS:
            y1, acc1, _ = dense_fwd(case, T, sn.poison(x, p["x"], kind), wt)
            sn.assert_propagates(y0, y1, d["fwd"], kind, f"conv_fwd {what} x {kind}", fam)
            if acc1 is not None:                         # every output channel holds a poisoned pixel: every sum goes
                assert all_bad(fold(acc1, cout), kind), f"{what}: statistics of poisoned channels stayed finite / not NaN ({kind})"
            y1, acc1, _ = dense_fwd(case, T, x, sn.poison(wt, p["w"], kind))
            sn.assert_propagates(y0, y1, d["fwd_w"], kind, f"conv_fwd {what} w {kind}", fam)
            if acc1 is not None:                         # one poisoned weight: exactly that output channel's two sums
                y_m = torch.where(d["fwd_w"], y0.cpu(), y1.cpu())
                sn.assert_propagates(fold(acc0, cout), fold(acc1, cout), d["stats_w"], kind, f"conv_fwd statistics {what} w {kind}", "conv_stats",
                                     bound=lambda merged: sc.assert_stats(merged, y_m, f"conv_fwd statistics {what}"))

        def run_fwd(hostile):
            y, acc, guards = dense_fwd(case, T, x, wt, hostile)
            if acc is not None:
                sc.assert_stats(fold(acc, cout), y, f"conv_fwd statistics {what} (NaN surroundings: {hostile})")
            return {"y": y}, guards
        sn.assert_unmoved_by_surroundings(run_fwd, f"conv_fwd {what}", fam)

        # ---- data gradient: plain, accumulate, two accumulate sources
        if case["dgrad"]:
            for form in ("plain", "acc") + (("acc2",) if s == 1 else ()):
                dep = d[{"plain": "dgrad", "acc": "dgrad_acc", "acc2": "dgrad_acc2"}[form]]
                dx0, _ = dense_dgrad(case, T, form, inp["dy"], wt, inp["base"], inp["acc2"])
                for kind in sn.KINDS:
                    base = sn.poison(inp["base"], p["base"], kind) if form != "plain" else inp["base"]
                    a2 = sn.poison(inp["acc2"], p["acc2"], kind) if form == "acc2" else inp["acc2"]
                    dx1, _ = dense_dgrad(case, T, form, sn.poison(inp["dy"], p["dy"], kind), wt, base, a2)
                    sn.assert_propagates(dx0, dx1, dep, kind, f"conv_dgrad {form} {what} {kind}", dfam)

                def run_dgrad(hostile, form=form):
                    dx, guards = dense_dgrad(case, T, form, inp["dy"], wt, inp["base"], inp["acc2"], hostile)
                    return {"dx": dx}, guards
                sn.assert_unmoved_by_surroundings(run_dgrad, f"conv_dgrad {form} {what}", dfam)

        # ---- fused inference epilogue: bias + SiLU + residual slice, and identity without residual
        if case["fused"]:
            for act, with_res in ((1, True), (0, False)):
                dep = d["fused"] if with_res else d["fwd"]
                f0, _ = dense_fused(case, T, act, with_res, x, wt, inp["bias"], inp["res"])
                for kind in sn.KINDS:
                    res = sn.poison(inp["res"], p["res"], kind)
                    f1, _ = dense_fused(case, T, act, with_res, sn.poison(x, p["x"], kind), wt, inp["bias"], res)
                    sn.assert_propagates(f0, f1, dep, kind, f"conv_fwd_act act={act} res={with_res} {what} {kind}", fam)

                def run_fused(hostile, act=act, with_res=with_res):
                    y, guards = dense_fused(case, T, act, with_res, x, wt, inp["bias"], inp["res"], hostile)
                    return {"y": y}, guards
                sn.assert_unmoved_by_surroundings(run_fused, f"conv_fwd_act act={act} {what}", fam)

        # ---- the weight gradient of the generic and fp32 kernels (atomics: EXEMPT)
        if fam in ("generic", "fp32"):
            check_wgrad(case, T, inp, p, d, fam + "_wgrad", f"conv_wgrad {what}")


def test_a_real_launch_that_reads_past_its_slice_is_rejected():
    """The harness itself, on the device: the gather kernel is handed 8 channels MORE than the layer has, against weights that
    are zero there -- the leak 'reads past Cin, cancelled by a zero weight'.  With the finite neighbours of the other modules
    the result is the layer's own, bit for bit; with NaN neighbours every output is 0 x NaN, and assert_unmoved_by_surroundings
    says so."""
    o = ops()
    case = nc.DENSE[0]
    cin, cout, k, s = case["cin"], case["cout"], case["k"], case["s"]
    inp = nc.dense_inputs(case, BF)
    wide = torch.cat([inp["w"], torch.zeros(cout, 8, k, k, dtype=BF)], 1)
    wp = o.pack_weights(wide.float().to(DEV), k, s, 0, BF)

    def run(hostile):
        _, (buf, off, hi) = place(inp["x"], cin + 32, NAN if hostile else 3.0)
        return {"y": o.conv_fwd(buf[:, off:off + cin + 8], wp, None, cout, k, s)}, [(buf, off, hi)]
    assert torch.equal(run(False)[0]["y"], dense_fwd(case, BF, inp["x"], inp["w"], stats=False)[0]), "finite neighbours x 0 must be invisible"
    fams, e = sn.failing(lambda: sn.assert_unmoved_by_surroundings(run, "reads 8 channels past Cin", "gather"))
    assert fams == ["gather"] and e.count == N * cout * case["h"] * case["w"], (fams, e and e.count)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("to,ti,pf,cin,cout,k,s", nc.WGRAD)
def test_weight_gradient_every_forced_tile(to, ti, pf, cin, cout, k, s, dtype):
    """the product path (partials + reduce, no atomics): the partials buffer and dw start as NaN in the surroundings launch"""
    lib().call("yolo_wgrad_tune_set", to, ti, 0, 0)
    lib().call("yolo_wgrad_tune_pf", pf)
    case = nc.wgrad_case(cin, cout, k, s)
    oh, ow = nc.out_hw(7, 11, k, s)
    plan = lib().query("yolo_conv2d_wgrad_plan", N, 7, 11, cin, oh, ow, cout, k, s, lib_dt(dtype))
    assert plan // 10000000 == pf and plan // 1000000 % 10 == to and plan // 100000 % 10 == ti, plan
    p, d = nc.dense_plan(case)
    check_wgrad(case, dtype, nc.dense_inputs(case, dtype), p, d, "wgrad", f"conv_wgrad {(to, ti, pf)} {case['id']} {str(dtype)[6:]}")


@pytest.mark.parametrize("cin,cout,k,s", nc.WGRAD_ATOMICS)
def test_weight_gradient_atomics_path(cin, cout, k, s, monkeypatch):
    """algo 3 (the first MFMA design, float atomics): outside dep held to the float64 reference at the family's constant"""
    monkeypatch.setattr(ops(), "ALGO", 3)
    case = nc.wgrad_case(cin, cout, k, s)
    p, d = nc.dense_plan(case)
    check_wgrad(case, BF, nc.dense_inputs(case, BF), p, d, "wgrad_atomics", f"conv_wgrad algo 3 {case['id']}")


# ------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
def test_stem_unfold_route_fused_forward_and_weight_gradients(dtype):
    o = ops()
    cout, h, w = nc.STEM["cout"], nc.STEM["h"], nc.STEM["w"]
    oh, ow = nc.out_hw(h, w, 3, 2)
    p, d = nc.stem_plan()
    img = nc.rnd((N, 3, h, w), 41, dtype=F32)
    wt = nc.rnd((cout, 3, 3, 3), 42, 0.2, dtype)
    dy = nc.rnd((N, cout, oh, ow), 43, dtype=dtype)
    wp = o.stem_pack_weights(wt.float().to(DEV), dtype)
    assert o.stem_conv_eligible(img.to(DEV), dtype, cout)
    what = f"stem {str(dtype)[6:]}"

    def unfold(im, hostile=False):
        with surroundings(hostile):
            return o.conv_fwd(o.stem_im2col(im.to(DEV), dtype), wp, None, cout, 1, 1)

    def fused(im, hostile=False):
        with surroundings(hostile):
            acc = o.bn_acc_new(cout, DEV)
            return o.stem_conv_fwd(im.to(DEV), wp, cout, dtype, acc), acc

    u0, (f0, acc0) = unfold(img), fused(img)
    for kind in sn.KINDS:
        bad = sn.poison(img, p["img"], kind)
        sn.assert_propagates(u0, unfold(bad), d["fwd"], kind, f"{what} im2col + 1x1 {kind}", "stem")
        f1, acc1 = fused(bad)
        sn.assert_propagates(f0, f1, d["fwd"], kind, f"{what} fused forward {kind}", "stem")
        assert all_bad(fold(acc1, cout), kind)
    sn.assert_unmoved_by_surroundings(lambda hostile: ({"y": unfold(img, hostile)}, []), f"{what} im2col + 1x1", "stem")
    sn.assert_unmoved_by_surroundings(lambda hostile: ({"y": fused(img, hostile)[0]}, []), f"{what} fused forward", "stem")

    # ---- fused stem_wgrad: NaN in image channel 1 -> dw[:, 1] (taps that exist); in dy channels -> dw[co]
    def wgrad(im, g, hostile=False):
        with surroundings(hostile):
            gd, guard = place(g, cout + 16, NAN if hostile else 3.0)
            return o.stem_wgrad(im.to(DEV), gd, F32), [guard]
    w0, _ = wgrad(img, dy)
    for kind in sn.KINDS:
        sn.assert_propagates(w0, wgrad(sn.poison(img, p["img_w"], kind), dy)[0], d["wgrad_img"], kind, f"{what} stem_wgrad image {kind}", "stem_wgrad")
        sn.assert_propagates(w0, wgrad(img, sn.poison(dy, p["dy_w"], kind))[0], d["wgrad_dy"], kind, f"{what} stem_wgrad dy {kind}", "stem_wgrad")

    def run_wgrad(hostile):
        dw, guards = wgrad(img, dy, hostile)
        return {"dw": dw}, guards
    sn.assert_unmoved_by_surroundings(run_wgrad, f"{what} stem_wgrad", "stem_wgrad")

    # ---- the one-pass stem backward (BatchNorm sums and weight gradient, no dz): poisoned dout channels -> dw[co], dgamma[co], dbeta[co]
    y = f0
    gamma, beta = (1 + 0.1 * nc.rnd((cout,), 44, dtype=F32)).to(DEV), (0.1 * nc.rnd((cout,), 45, dtype=F32)).to(DEV)
    mean, invstd, scale, shift = o.bn_train_stats(y, gamma, beta, torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV), 0.03, 1e-3)

    def one_pass(im, g, hostile=False):
        with surroundings(hostile):
            gd, guard = place(g, cout + 16, NAN if hostile else 3.0)
            dw, dga, dbe = o.stem_bn_wgrad(im.to(DEV), gd, y, scale, shift, mean, invstd, gamma, 1, F32)
        return {"dw": dw, "dgamma": dga, "dbeta": dbe}, [guard]
    r0, _ = one_pass(img, dy)
    for kind in sn.KINDS:
        r1, _ = one_pass(img, sn.poison(dy, p["dy_w"], kind))
        sn.assert_propagates(r0["dw"], r1["dw"], d["wgrad_dy"], kind, f"{what} one-pass backward dw {kind}", "stem_wgrad")
        sn.assert_propagates(r0["dgamma"], r1["dgamma"], d["chan_dy"], kind, f"{what} one-pass backward dgamma {kind}", "stem_wgrad")
        sn.assert_propagates(r0["dbeta"], r1["dbeta"], d["chan_dy"], kind, f"{what} one-pass backward dbeta {kind}", "stem_wgrad")
        r1, _ = one_pass(sn.poison(img, p["img_w"], kind), dy)
        sn.assert_propagates(r0["dw"], r1["dw"], d["wgrad_img"], kind, f"{what} one-pass backward dw, image {kind}", "stem_wgrad")
        for key in ("dgamma", "dbeta"):                  # neither reads the image
            assert torch.equal(r0[key], r1[key]), key
    sn.assert_unmoved_by_surroundings(lambda hostile: one_pass(img, dy, hostile), f"{what} one-pass backward", "stem_wgrad")


# ------------------------------------------------------------------------------------------------- depthwise
def dw_launches(c, h, w, dtype, inp, padx, pady, hostile=False):
    o = ops()
    fill = NAN if hostile else 7.0
    w9, bias = inp["w9"].to(DEV), inp["bias"].to(DEV)
    r = {}
    with surroundings(hostile):
        x, gx = place(inp["x"], c + 16 * padx, fill)
        dy, gdy = place(inp["dy"], c + 16 * pady, fill)
        r["fwd"] = o.dw_fwd(x, w9)
        acc = o.bn_acc_new(c, DEV)
        r["fwd_stats"] = o.dw_fwd(x, w9, acc)
        for act in (0, 1):
            y = o.dw_fwd_act(x, w9, bias, act)
            if y is not None:                            # fp32 / unaligned channel counts: not taken, by contract
                r[f"act{act}"] = y
        r["dgrad"] = o.dw_dgrad(dy, w9)
        base, gb = place(inp["base"], c + 16, fill)
        r["dgrad_acc"] = o.dw_dgrad(dy, w9, acc_into=base)
        r["wgrad"] = o.dw_wgrad(x, dy)                   # `part` and dw come from the allocator: NaN-prefilled when hostile
    return r, acc, [gx, gdy, gb]


def check_dw(c, h, w, padx, pady, dtype, family, variant):
    p, d = nc.dw_plan(c, h, w)
    inp = nc.dw_inputs(c, h, w, dtype)
    sn.require_nonzero(f"dw {c}x{h}x{w}", w9=inp["w9"], x=inp["x"], dy=inp["dy"])
    what = f"depthwise {family} {c}x{h}x{w} {str(dtype)[6:]}"
    r0, acc0, _ = dw_launches(c, h, w, dtype, inp, padx, pady)
    if variant:
        assert set(r0) >= {"act0", "act1"}, "dw_fwd_act did not take an aligned 16-bit tensor"
    for kind in sn.KINDS:
        bad = dict(inp, x=sn.poison(inp["x"], p["x"], kind), dy=sn.poison(inp["dy"], p["dy"], kind), base=sn.poison(inp["base"], p["base"], kind))
        r1, acc1, _ = dw_launches(c, h, w, dtype, bad, padx, pady)
        for key in r0:
            if key == "wgrad":
                continue
            dep = d["dgrad_acc"] if key == "dgrad_acc" else d["dgrad"] if key == "dgrad" else d["fwd"]
            sn.assert_propagates(r0[key], r1[key], dep, kind, f"{what} {key} {kind}", family)
        y_m = torch.where(d["fwd"], r0["fwd_stats"].cpu(), r1["fwd_stats"].cpu())
        stats_ref = sb.sums_fwd(y_m, dtype)

        def stats_bound(merged):
            sb.assert_within(merged[0].float(), stats_ref["s"], F32, f"{what} statistics sum", "bn_sum")
            sb.assert_within(merged[1].float(), stats_ref["q"], F32, f"{what} statistics sumsq", "bn_sumsq")
        sn.assert_propagates(fold(acc0, c), fold(acc1, c), d["stats"], kind, f"{what} statistics {kind}", "depthwise_stats", bound=stats_bound)
        # the weight gradient: x poisoned alone, then dy alone
        rx, _, _ = dw_launches(c, h, w, dtype, dict(inp, x=bad["x"]), padx, pady)
        taps = d["taps"]                                # (3, 3): the taps that meet an output pixel at all (nonfinite_cases.dw_plan)
        sn.assert_propagates(r0["wgrad"][:, :, taps], rx["wgrad"][:, :, taps], d["wgrad_x"], kind, f"{what} wgrad x {kind}", family + "_wgrad")
        ry, _, _ = dw_launches(c, h, w, dtype, dict(inp, dy=bad["dy"]), padx, pady)
        sn.assert_propagates(r0["wgrad"][:, :, taps], ry["wgrad"][:, :, taps], d["wgrad_dy"], kind, f"{what} wgrad dy {kind}", family + "_wgrad")

    def run(hostile):
        r, acc, guards = dw_launches(c, h, w, dtype, inp, padx, pady, hostile)
        s_ref = sb.sums_fwd(r["fwd_stats"], dtype)
        s, q = sb.fold(acc, c)
        sb.assert_within(s.float(), s_ref["s"], F32, f"{what} statistics sum", "bn_sum")
        sb.assert_within(q.float(), s_ref["q"], F32, f"{what} statistics sumsq", "bn_sumsq")
        return r, guards
    sn.assert_unmoved_by_surroundings(run, what, family)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("variant", [1, 2], ids=["strip", "rows"])
@pytest.mark.parametrize("c,h,w,padx,pady", nc.DW)
def test_depthwise_strip_and_rows_kernels(c, h, w, padx, pady, variant, dtype):
    lib().call("yolo_dw_tune_set", variant)
    want = 1 if variant == 2 else 2
    assert lib().query("yolo_dw_plan", N, h, w, c, 0) == want and lib().query("yolo_dw_plan", N, h, w, c, 12) == want
    check_dw(c, h, w, padx, pady, dtype, "depthwise", variant)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_depthwise_generic_kernel(dtype):
    c, h, w, padx, pady = nc.DW_GENERIC
    assert lib().query("yolo_dw_plan", N, h, w, c, 0) == 0
    check_dw(c, h, w, padx, pady, dtype, "depthwise", 0)


# ------------------------------------------------------------------------------------------------- BatchNorm
def bn_dev(t, pad, fill):
    """pad / 2 channels into a buffer of c + pad channels, as tests/test_gpu_bn.py places its tensors (2 channels in: no
    16-byte packets for any type)"""
    return place(t, t.shape[1] + pad, fill, off=pad // 2)


def bn_deterministic(case, y, dout, pad, hostile=False):
    """bn_train_stats -> bn_act_fwd -> bn_act_bwd / bn_act_bwd_eval (no atomics: bit-reproducible)"""
    o = ops()
    fill = NAN if hostile else 7.0
    gamma, beta = case.gamma.to(DEV), case.beta.to(DEV)
    with surroundings(hostile):
        yd, gy = bn_dev(y, pad, fill)
        dd, gd = bn_dev(dout, pad, fill)
        res = None if case.res is None else bn_dev(case.res, 0, fill)[0]
        rm, rv = case.rmean.to(DEV), case.rvar.to(DEV)
        mean, invstd, scale, shift = o.bn_train_stats(yd, gamma, beta, rm, rv, case.momentum, case.eps)
        r = {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "rmean": rm, "rvar": rv,
             "out": o.bn_act_fwd(yd, scale, shift, case.act, res)}
        r["dy"], r["dgamma"], r["dbeta"] = o.bn_act_bwd(dd, yd, scale, shift, mean, invstd, gamma, case.act)
    return r, [gy, gd]


def bn_accumulator(case, y, dout, pad):
    """bn_stats_acc -> bn_act_fwd_train -> bn_act_bwd_train (float atomics: EXEMPT family bn_acc)"""
    o = ops()
    n, c, h, w = case.shape
    gamma, beta = case.gamma.to(DEV), case.beta.to(DEV)
    yd, dd = bn_dev(y, pad, 7.0)[0], bn_dev(dout, pad, 7.0)[0]
    res = None if case.res is None else bn_dev(case.res, 0, 7.0)[0]
    acc_f, acc_b = o.bn_acc_new(c, DEV), o.bn_acc_new(c, DEV)
    o.bn_stats_acc(yd, acc_f)
    rm, rv = case.rmean.to(DEV), case.rvar.to(DEV)
    out, mean, invstd, scale, shift = o.bn_act_fwd_train(yd, acc_f, gamma, beta, rm, rv, case.momentum, case.eps, case.act, res)
    dy, dgamma, dbeta = o.bn_act_bwd_train(dd, yd, scale, shift, mean, invstd, gamma, case.act, acc_b)
    return {"acc_f": acc_f.view(-1, 2, c), "acc_b": acc_b.view(-1, 2, c), "mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "rmean": rm, "rvar": rv,
            "out": out, "dy": dy, "dgamma": dgamma, "dbeta": dbeta}


FWD_KEYS = ("mean", "invstd", "scale", "shift", "rmean", "rvar", "out")
BWD_KEYS = ("dy", "dgamma", "dbeta")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", nc.BN, ids=lambda s: "x".join(map(str, s[:4])) + f"+{s[4]}")
def test_batchnorm_training_passes(shape, dtype, act):
    """NaN, then +inf, in ONE element of channel c: the training statistics, the running statistics, the coefficients and the
    output of exactly channel c go NaN (with +inf: non-finite -- the mean is +inf, the variance inf - inf); NaN / inf in dout:
    exactly dgamma[c], dbeta[c] and dy[:, c].  SiLU and a residual where the shape has one."""
    n, c, h, w, pad, with_res = shape
    case = sb.Case("plain", n, c, h, w, dtype, act, with_res)
    pos, chan, full = nc.bn_plan(n, c, h, w)
    sn.require_nonzero(case.what, gamma=case.gamma)

    def dep_of(t):
        return full if t.dim() == 4 else chan

    r0, _ = bn_deterministic(case, case.y, case.dout, pad)
    a0 = bn_accumulator(case, case.y, case.dout, pad)
    # what a poisoned y reaches: everything of the channel but dbeta = sum dz without SiLU (dz = dout then)
    hit_y = FWD_KEYS + (BWD_KEYS if act else ("dy", "dgamma"))
    for kind in sn.KINDS:
        # ---- the deterministic path (no atomics): y poisoned (the backward reads the poisoned y too), then dout poisoned
        r1, _ = bn_deterministic(case, sn.poison(case.y, pos, kind), case.dout, pad)
        for key in hit_y:
            sn.assert_propagates(r0[key], r1[key], dep_of(r0[key]), kind, f"{case.what} deterministic {key}, y {kind}", "bn_det")
        if not act:
            assert torch.equal(r0["dbeta"], r1["dbeta"]), "dbeta without an activation does not read y"
        r1, _ = bn_deterministic(case, case.y, sn.poison(case.dout, pos, kind), pad)
        for key in FWD_KEYS:
            assert torch.equal(r0[key], r1[key]), key
        for key in BWD_KEYS:
            sn.assert_propagates(r0[key], r1[key], dep_of(r0[key]), kind, f"{case.what} deterministic {key}, dout {kind}", "bn_det")
        # ---- the accumulator path (float atomics, EXEMPT): the path 'poisoned outside dep, clean inside' is verified stage by
        # stage by strict_bn from the clean case -- once per run, it is the bound of every tensor of the run
        for which, yy, dd, hit in (("y", sn.poison(case.y, pos, kind), case.dout, hit_y + ("acc_f", "acc_b")),
                                   ("dout", case.y, sn.poison(case.dout, pos, kind), BWD_KEYS + ("acc_b",))):
            a1 = bn_accumulator(case, yy, dd, pad)
            deps = {key: chan.view(1, c).expand(2, c) if key.startswith("acc") else dep_of(a0[key]) for key in a0}
            deps = {key: m.clone() if key in hit else torch.zeros_like(m) for key, m in deps.items()}
            if which == "y" and not act:
                deps["acc_b"][0] = False                 # sum dz = sum dout does not read y; sum dz y does
            # the accumulators are [8][2][C] replicas: merged replica by replica for strict_bn (it folds them in float64),
            # compared folded (the poisoned sum sits in the one replica its workgroup adds to)
            merged = {key: torch.where(deps[key].expand_as(a0[key]) if key.startswith("acc") else deps[key], a0[key].cpu(), a1[key].cpu())
                      for key in a0}
            a0f, a1f = ({key: v.sum(0) if key.startswith("acc") else v for key, v in a.items()} for a in (a0, a1))
            verified = []

            def bound(_merged_tensor):
                if not verified:
                    sb.verify_accumulator_path(case, merged)
                    verified.append(True)
            for key in hit:
                sn.assert_propagates(a0f[key], a1f[key], deps[key], kind, f"{case.what} accumulator {key}, {which} {kind}", "bn_acc", bound)
            for key in a0:
                if key not in hit:                       # not reached: finite, and inside the verified path
                    assert bool(torch.isfinite(a1[key].double()).all()), f"{case.what} accumulator {key}, {which} {kind}: leaked"

    def run(hostile):
        r, guards = bn_deterministic(case, case.y, case.dout, pad, hostile)
        return r, guards
    sn.assert_unmoved_by_surroundings(run, f"{case.what} deterministic", "bn_det")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
def test_batchnorm_eval_passes_touch_only_the_poisoned_element(dtype, act):
    o = ops()
    n, c, h, w, pad, _ = nc.BN[1]
    case = sb.Case("plain", n, c, h, w, dtype, act, True)
    pos = nc.positions(n, c, h, w, c - 3)
    dep = sn.indicator((n, c, h, w), pos) > 0
    scale, shift = o.bn_eval_coeffs(case.gamma.to(DEV), case.beta.to(DEV), case.rmean.to(DEV), case.rvar.to(DEV), case.eps)

    def run(y, dout, res, hostile=False):
        fill = NAN if hostile else 7.0
        with surroundings(hostile):
            yd, gy = bn_dev(y, pad, fill)
            dd, gd = bn_dev(dout, pad, fill)
            rd, gr = bn_dev(res, pad, fill)
            ob = o.new_nhwc(n, c + 16, h, w, dtype, DEV).fill_(fill)
            r = {"out": o.bn_act_fwd(yd, scale, shift, act, rd, out=ob[:, 8:8 + c]), "dy": o.bn_act_bwd_eval(dd, yd, scale, shift, act)}
        return r, [gy, gd, gr, (ob, 8, 8 + c)]
    r0, _ = run(case.y, case.dout, case.res)
    for kind in sn.KINDS:
        r1, _ = run(sn.poison(case.y, pos, kind), case.dout, case.res)
        sn.assert_propagates(r0["out"], r1["out"], dep, kind, f"bn_act_fwd y {kind} {case.what}", "bn_det")
        sn.assert_propagates(r0["dy"], r1["dy"], dep, kind, f"bn_act_bwd_eval y {kind} {case.what}", "bn_det")
        r1, _ = run(case.y, sn.poison(case.dout, pos, kind), sn.poison(case.res, pos[:2], kind))
        sn.assert_propagates(r0["out"], r1["out"], sn.indicator((n, c, h, w), pos[:2]) > 0, kind, f"bn_act_fwd res {kind} {case.what}", "bn_det")
        sn.assert_propagates(r0["dy"], r1["dy"], dep, kind, f"bn_act_bwd_eval dout {kind} {case.what}", "bn_det")
    sn.assert_unmoved_by_surroundings(lambda hostile: run(case.y, case.dout, case.res, hostile), f"bn eval {case.what}", "bn_det")


def _type_max(dtype):
    return float(torch.finfo(dtype).max)


@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
def test_activation_at_the_ends_of_the_range(dtype):
    """act_fwd / act_grad (bn_act_fwd / bn_act_bwd_eval with scale 1, shift 0, SiLU) at z = +-max finite and +-88, +-89, +-104,
    where __expf overflows and the reciprocal goes subnormal: finite, and inside the E_act rule of strict_bn against float64
    silu / silu'; z = -inf -> NaN, z = +inf -> +inf, as in torch."""
    o = ops()
    big = _type_max(dtype)
    zs = [big, -big, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1.0, -1.0, float("inf"), float("-inf")]
    c = 8
    z = torch.tensor(zs + [0.5] * (16 - len(zs))).to(dtype).view(1, 2, 1, c).permute(0, 3, 1, 2).contiguous()      # (1, 8, 2, 1)
    zd = place(z)[0]
    one, zero = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    out = o.bn_act_fwd(zd, one, zero, 1).cpu()
    dout = torch.ones_like(z)
    grad = o.bn_act_bwd_eval(place(dout)[0], zd, one, zero, 1).cpu()
    fin = torch.isfinite(z)
    assert bool(torch.isfinite(out[fin]).all()) and bool(torch.isfinite(grad[fin]).all()), (out[fin], grad[fin])
    zf = torch.where(fin, z, torch.ones_like(z))
    ref_o, noise_o = sb.fwd_apply(zf, one.cpu(), zero.cpu(), 1)
    dz, ddz, _ = sb.bwd_dz(torch.ones_like(zf), zf, one.cpu(), zero.cpu(), 1)
    ref_g, noise_g = sb.bwd_apply(dz, ddz, zf, one.cpu())
    sb.assert_within(torch.where(fin, out, ref_o.to(dtype)), (ref_o, noise_o), dtype, f"act_fwd at the range ends {dtype}", "bn_fwd")
    sb.assert_within(torch.where(fin, grad, ref_g.to(dtype)), (ref_g, noise_g), dtype, f"act_grad at the range ends {dtype}", "bn_dy")
    pinf, ninf = (z == float("inf")), (z == float("-inf"))
    want = torch.nn.functional.silu(z.float())
    assert bool((out[pinf].float() == float("inf")).all()) and bool(torch.isinf(want[pinf]).all())
    assert bool(torch.isnan(out[ninf]).all()) and bool(torch.isnan(want[ninf]).all())


# ------------------------------------------------------------------------------------------------- attention
def _merge(mask, n, hw):
    """(B, T, d) mask -> (N, heads * d, H, W) element mask"""
    return sa.merge(mask.double(), n, *hw) > 0


def _stash_cmp(stash, route, b, t, dtype):
    """the comparable part of a stash: the fp32 row log-sum-exp (B, T), or the stashed probabilities (B, T, T) without the pad columns"""
    if route != "gemm":
        return stash.view(torch.float32).reshape(b, t).cpu()
    tp = (t + 31) // 32 * 32
    return stash.view(dtype).reshape(b, t, tp)[..., :t].cpu()


def _attn_poison(which, rows, heads, dk, dh, hw):
    """-> (position in the (N, heads * (2 dk + dh), H, W) tensor, keyword of attention_dep) of the case's q / k / v poison"""
    r = rows[which]
    prob, tok, comp = r if len(r) == 3 else r + (3,)
    pos = (prob // heads, nc.attn_channel(which, prob % heads, comp, heads, dk, dh), tok // hw[1], tok % hw[1])
    return pos, ({"v_elems": [r]} if which == "v" else {f"{which}_rows": [r]})


def _head_pos(elem, heads, dh, hw):
    """(problem, token, component) -> position in an (N, heads * dh, H, W) tensor (o, dO, d_vp, the re-gathered v)"""
    prob, tok, comp = elem
    return (prob // heads, (prob % heads) * dh + comp, tok // hw[1], tok % hw[1])


@pytest.mark.parametrize("route,dtype,heads,dk,dh,t", nc.ATTN, ids=[f"{r}-{str(d)[6:]}-dk{k}-T{t}" for r, d, _, k, _, t in nc.ATTN])
def test_attention_forward_stash_and_backward(route, dtype, heads, dk, dh, t):
    """A NaN in one query row: that output row and its lse / stash row; in one key row: every row of that (image, head),
    nothing of any other; in one component of a value row: that component of every row of the (image, head); dO likewise into
    dQ (its row), dK (the whole (image, head)) and dV (its component); d_vp: its element of dV.  +inf goes into q, v, dO and
    d_vp (a key at -inf is a masked key: its rows stay finite, legitimately -- so k gets NaN only)."""
    o = ops()
    n, b, scale, hw = nc.ATTN_N, nc.ATTN_N * heads, dk ** -0.5, sa.hw(t)
    qkv = sn.fix_zeros(sa.make_qkv(n, heads, dk, dh, t, "plain", 60 + t, dtype))
    d_o = nc.rnd((n, heads * dh) + hw, 51, dtype=dtype)
    d_vp = nc.rnd((n, heads * dh) + hw, 52, dtype=dtype)
    rows = nc.attn_plan(heads, t)
    what = f"attention {route} {str(dtype)[6:]} T={t}"
    fam = f"attn_{route}"

    def fwd(x, hostile=False):
        with surroundings(hostile):
            xd, g = place(x, x.shape[1] + 16, NAN if hostile else 7.0)
            og, vg, stash = o.attn_fwd(xd, heads, dk, dh, scale)
        return xd, og, vg, stash, [g]

    def bwd(xd, og, stash, g_o, g_vp, hostile=False):
        with surroundings(hostile):
            fill = NAN if hostile else 7.0
            god, g1 = place(g_o, g_o.shape[1] + 16, fill)
            gvd, g2 = place(g_vp, g_vp.shape[1] + 16, fill)
            return o.attn_bwd(xd, og, god, gvd, stash, heads, dk, dh, scale), [g1, g2]

    def qkv_mask(dep):
        return _merge(torch.cat([dep["dq"], dep["dk"], dep["dv"]], 2), n, hw)

    xd0, o0, v0, st0, _ = fwd(qkv)
    got_route = "fp32" if dtype == F32 else "fused" if st0.numel() == b * t * 4 else "gemm"
    assert got_route == route, (got_route, route)
    dq0, _ = bwd(xd0, o0, st0, d_o, d_vp)
    s0 = _stash_cmp(st0, route, b, t, dtype)

    for which, kinds in (("q", sn.KINDS), ("k", ("nan",)), ("v", sn.KINDS)):
        pos, kw = _attn_poison(which, rows, heads, dk, dh, hw)
        dep = sn.attention_dep(b, t, dk, dh, **kw)
        for kind in kinds:
            xd1, o1, v1, st1, _ = fwd(sn.poison(qkv, [pos], kind))
            sn.assert_propagates(o0, o1, _merge(dep["o"], n, hw), kind, f"{what} o, {which} {kind}", fam)
            s1 = _stash_cmp(st1, route, b, t, dtype)
            if which != "v":
                sdep = dep["lse"] if s0.dim() == 2 else dep["lse"].view(b, t, 1).expand(b, t, t)
                sn.assert_propagates(s0, s1, sdep, kind, f"{what} stash, {which} {kind}", fam)
                assert torch.equal(v0, v1), f"{what}: the re-gathered v depends on {which}"
            else:
                assert torch.equal(s0, s1), f"{what}: the stash depends on v"
                vdep = sn.indicator(tuple(v0.shape), [_head_pos(rows["v"], heads, dh, hw)]) > 0
                sn.assert_propagates(v0, v1, vdep, kind, f"{what} re-gathered v, {kind}", fam)
            if kind == "nan":                            # the backward from the poisoned forward's own o and stash
                dq1, _ = bwd(xd1, o1, st1, d_o, d_vp)
                sn.assert_propagates(dq0, dq1, qkv_mask(dep), kind, f"{what} dqkv, {which} {kind}", fam)
    dep = sn.attention_dep(b, t, dk, dh, do_elems=[rows["do"]], dvp_elems=[rows["dvp"]])
    for kind in sn.KINDS:
        g_bad = sn.poison(d_o, [_head_pos(rows["do"], heads, dh, hw)], kind)
        dq1, _ = bwd(xd0, o0, st0, g_bad, sn.poison(d_vp, [_head_pos(rows["dvp"], heads, dh, hw)], kind))
        sn.assert_propagates(dq0, dq1, qkv_mask(dep), kind, f"{what} dqkv, dO and d_vp {kind}", fam)

    def run(hostile):
        xd, og, vg, stash, guards = fwd(qkv, hostile)
        dq, g2 = bwd(xd, og, stash, d_o, d_vp, hostile)
        return {"o": og, "vp": vg, "stash": _stash_cmp(stash, route, b, t, dtype), "dqkv": dq}, guards + g2
    sn.assert_unmoved_by_surroundings(run, what, fam)


@pytest.mark.parametrize("route,dtype,heads,dk,dh,t", nc.ATTN_NOGRAD, ids=[f"{r}-{str(d)[6:]}-T{t}" for r, d, _, _, _, t in nc.ATTN_NOGRAD])
def test_attention_forward_without_stash(route, dtype, heads, dk, dh, t):
    """attn_fwd_nograd: the one-image kernel (36 tokens) and the key-blocked kernel (449: one full key block and 193 keys)"""
    o = ops()
    n, b, scale, hw = nc.ATTN_N, nc.ATTN_N * heads, dk ** -0.5, sa.hw(t)
    qkv = sn.fix_zeros(sa.make_qkv(n, heads, dk, dh, t, "plain", 100 + t, dtype))
    rows = nc.attn_plan(heads, t)
    what = f"attention (no stash) {route} {str(dtype)[6:]} T={t}"

    def fwd(x, hostile=False):
        with surroundings(hostile):
            xd, g = place(x, x.shape[1] + 16, NAN if hostile else 7.0)
            got = o.attn_fwd_nograd(xd, heads, dk, dh, scale)
        assert got is not None
        return got[0], got[1], [g]
    o0, v0, _ = fwd(qkv)
    for which, kinds in (("q", sn.KINDS), ("k", ("nan",)), ("v", sn.KINDS)):
        pos, kw = _attn_poison(which, rows, heads, dk, dh, hw)
        dep = sn.attention_dep(b, t, dk, dh, **kw)
        for kind in kinds:
            o1, v1, _ = fwd(sn.poison(qkv, [pos], kind))
            sn.assert_propagates(o0, o1, _merge(dep["o"], n, hw), kind, f"{what} o, {which} {kind}", f"attn_{route}")
            if which != "v":
                assert torch.equal(v0, v1)

    def run(hostile):
        og, vg, guards = fwd(qkv, hostile)
        return {"o": og, "vp": vg}, guards
    sn.assert_unmoved_by_surroundings(run, what, f"attn_{route}")


# ------------------------------------------------------------------------------------------------- f16 store overflow
F16_MAX = 65504.0
# The model test's initial loss scale.  At 32 x 32 the stride-32 level is ONE pixel: its BatchNorms normalise two values per
# channel (invstd up to eps^-1/2 = 31.6 per layer), and the backward of a CLEAN step overflows f16 on its own at ordinary
# scales -- measured on the MI355X: skipped at 256 and 128, at 1 and 0.5 after one update, finite at 64 / 0.25 and below,
# while 64 x 64 is finite at 256.  2^-10 leaves that a factor of 256; AdamW's update does not depend on the gradient's scale.
SCALE0 = 2.0 ** -10


@pytest.mark.parametrize("tune,plan", [((32, -1, 0, 0, 0, 0, 0, 0), 1032), ((128, -1, 0, 1, 0, 0, 0, 0), 1128),
                                       ((64, -1, 0, -1, 1, 64, 3, 64), nc.ring_plan(64, 64)), ((128, -1, 0, -1, 1, 128, 2, 32), nc.ring_plan(128, 128))],
                         ids=["gather-bn32-registers", "gather-bn128-dma", "ring-64x64", "ring-128x128-bk32"])
def test_f16_store_overflow_dense(tune, plan):
    """1x1 conv, 256 source channels, x = 256, every weight 1: the exact sum 65536 is above f16's largest finite value and
    its rounding boundary (65520): stored as +inf.  One input lowered to 224: 65504, stored exactly.  x = -256: -inf.
    Every product and partial sum is exact in fp32 (integers below 2^24): derived, no tolerance."""
    o = ops()
    cin, cout, h, w = 256, 72, 7, 11
    lib().call("yolo_conv_tune_set", *tune)
    got = lib().query("yolo_conv2d_plan", N, h, w, cin, h, w, cout, 1, 1, 0, 0, lib().F16)
    assert got == plan, f"test does not reach the variant it is written for: plan {got}, wanted {plan}"
    wp = o.pack_weights(torch.ones(cout, cin, 1, 1, device=DEV), 1, 1, 0, HF)
    x = torch.full((N, cin, h, w), 256.0, dtype=HF)
    x[1] = -256.0
    x[2, cin - 3] = 224.0
    y = o.conv_fwd(place(x, cin + 32)[0], wp, None, cout, 1, 1).float().cpu()
    assert bool((y[0] == float("inf")).all()), "65536 was not stored as +inf"
    assert bool((y[1] == float("-inf")).all()), "-65536 was not stored as -inf"
    assert bool((y[2] == F16_MAX).all()), f"65504 was not stored exactly: {y[2].unique().tolist()[:8]}"
    yf = o.conv_fwd_act(place(x, cin + 32)[0], wp, torch.zeros(cout, device=DEV), cout, 1, 1, 0)
    assert yf is not None, "no MFMA kernel took this shape"
    yf = yf.float().cpu()
    assert torch.equal(torch.nan_to_num(yf, posinf=1e9, neginf=-1e9), torch.nan_to_num(y, posinf=1e9, neginf=-1e9)), "fused epilogue stores differently"


@pytest.mark.parametrize("variant", [1, 2], ids=["strip", "rows"])
def test_f16_store_overflow_depthwise_and_bn(variant):
    """depthwise: nine taps of 8192 x 1.0 = 73728 -> +inf at interior pixels; 8192 x 1.0 with the centre row's taps only (a
    one-row map: 3 taps = 24576) stays finite and exact; bn_act_fwd: scale * y past 65504 -> +-inf, 65504 itself exact."""
    o = ops()
    c, h, w = 16, 5, 6
    lib().call("yolo_dw_tune_set", variant)
    w9 = torch.ones(c, 9, device=DEV)
    x = torch.full((N, c, h, w), 8192.0, dtype=HF)
    x[1] = -8192.0
    y = o.dw_fwd(place(x, c + 16)[0], w9).float().cpu()
    taps = torch.nn.functional.conv2d(torch.ones(1, 1, h, w), torch.ones(1, 1, 3, 3), padding=1)[0, 0]       # 4, 6 or 9 taps
    want = (taps * 8192.0).view(1, 1, h, w).expand(N, c, h, w).clone()
    want[1] = -want[1]
    want = want.to(HF).float()                                                                                # 32768, 49152 exact; 73728 -> inf
    assert bool(torch.isinf(want[0, 0, 2, 2])) and bool(torch.isfinite(want[0, 0, 0, 0]))
    assert torch.equal(y, want), "depthwise f16 store: overflow not stored as +-inf, or a finite sum not exact"
    lib().call("yolo_dw_tune_set", 0)
    yb = torch.tensor([32768.0, -32768.0, 32752.0, 1.0] * 4, dtype=HF).view(1, 1, 2, 8).permute(0, 3, 1, 2).contiguous()
    scale = torch.tensor([2.0, 2.0, 2.0, 65504.0, 2.0, 2.0, 2.0, 65504.0], device=DEV)
    out = o.bn_act_fwd(place(yb)[0], scale, torch.zeros(8, device=DEV), 0).float().cpu()
    want = (yb.double() * scale.cpu().double().view(1, 8, 1, 1)).to(HF).float()
    assert torch.equal(out, want) and bool(torch.isinf(want).any()) and bool((want == F16_MAX).any()), (out.flatten(), want.flatten())


# ------------------------------------------------------------------------------------------------- the model
def _snapshot(model, opt):
    ps = [p for p in model.parameters() if p.requires_grad]
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [v.clone() for v in opt.state[p].values() if torch.is_tensor(v)]
        out.append(opt.ema_shadow(p).clone())
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(sn.sm.bits(x), sn.sm.bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("route", ["plain", "clipped"])
def test_captured_fp16_step_skips_on_an_overflow_inside_the_model(route):
    """The overflow arises in the forward, not in .grad: one backbone conv weight is scaled until its f16 activations are inf.
    Both ways the device scaler learns of it (tests/test_gpu_adamw.py: plain -- k_found_inf reads the gradients; clipped --
    the global-norm pass k_grad_sqnorm does); a captured step through CapturedTraining never uses torch's GradScaler.
    NANO at 32 x 32, the smallest input the stride-32 level allows.  Deterministic mode, so that a twin model that never saw
    the overflow can be compared bit for bit."""
    from oracle import blocks as ob
    from src.hipops import functions as F_
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training.fused_adamw import DeviceGradScaler, HipAdamW
    from src.training.train_model import CapturedTraining
    o = ops()
    g = torch.Generator().manual_seed(7)
    img = torch.randn(2, 3, 32, 32, generator=g).cuda()
    gts = [torch.tensor([[16., 14., 12., 10., 3.]]), torch.tensor([[10., 20., 8., 14., 17.], [22., 9., 10., 12., 5.]])]

    def make():
        torch.manual_seed(0)
        model = Model(**ob.PRESETS["n"], num_classes=80).cuda().train()
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0 if route == "clipped" else None,
                       ema_decay=0.9, ema_tau=3.0)
        opt.device_amp = DeviceGradScaler("cuda", init_scale=SCALE0, growth_interval=1000)
        ct = CapturedTraining(model, YoloDFLQFLoss(num_classes=80), opt, "float16")
        assert ct.usable
        return model, opt, ct

    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert F_.deterministic_stats()
        (model, opt, ct), (twin, topt, tct) = make(), make()
        amp, tamp = opt.device_amp, topt.device_amp
        for c in (ct, tct):
            c.step(img, gts)                             # the eager warm-up step and the capture
            assert c.captured and c.runner.graph is not None and c.runner.opt_in_graph
        # (a) a clean replay: the weights change, nothing is skipped, and the twin follows bit for bit
        before = _snapshot(model, opt)
        ct.step(img, gts), tct.step(img, gts)
        torch.cuda.synchronize()
        assert not amp.last_step_skipped() and amp.get_scale() == SCALE0
        after_clean = _snapshot(model, opt)
        assert not _same(before, after_clean), "a clean captured step changed nothing"
        assert _same(after_clean, _snapshot(twin, topt)), "two identical models differ after a clean step: the twin proves nothing"
        # (b) the stem's weight scaled: its activations overflow f16
        wt = model.net.p1[0].conv.weight
        saved = wt.detach().clone()
        with torch.no_grad():
            wt.mul_(2.0 ** 17)
        assert float(wt.detach().abs().max()) < F16_MAX, "the scaled weight itself must stay finite in f16: the overflow is the activations'"
        cout = wt.shape[0]
        if o.stem_conv_eligible(img, HF, cout):
            act = o.stem_conv_fwd(img, o.stem_pack_weights(wt.detach(), HF), cout, HF)
        else:
            act = o.conv_fwd(o.stem_im2col(img, HF), o.stem_pack_weights(wt.detach(), HF), None, cout, 1, 1)
        assert bool(torch.isinf(act).any()), "the scaled weight did not overflow the f16 forward: the test is void"
        before = _snapshot(model, opt)
        ct.step(img, gts)
        torch.cuda.synchronize()
        assert amp.last_step_skipped(), "an overflow inside the forward did not reach the gradients: the step was not skipped"
        assert amp.get_scale() == 0.5 * SCALE0, amp.get_scale()
        with torch.no_grad():
            wt.copy_(saved)
        assert _same(before[1:], _snapshot(model, opt)[1:]), "a skipped step changed a parameter, an optimizer state or an EMA shadow"
        assert _same(after_clean, _snapshot(model, opt)), "the restored weight is not the weight from before"
        # (c) restored: the next replay equals the twin's step at the backed-off scale
        with torch.no_grad():
            tamp.state[0] = 0.5 * SCALE0
        ct.step(img, gts), tct.step(img, gts)
        torch.cuda.synchronize()
        assert not amp.last_step_skipped() and not tamp.last_step_skipped()
        now = _snapshot(model, opt)
        assert not _same(after_clean, now), "the step after the skipped one changed nothing"
        assert _same(now, _snapshot(twin, topt)), "the step after a skipped one differs from a model that never overflowed"
    finally:
        torch.use_deterministic_algorithms(False)
