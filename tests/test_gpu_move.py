"""-m gpu: the memory-bound kernels (k_maxpool5_fwd / _bwd, k_upsample2x_fwd / _bwd, k_copy_channels, k_add_n, the layout
transposes, k_multi_copy, k_pack_tiles) held to tests/strict_move.py: the exact class bit for bit (the pool's argmax
included), the sum class inside 1/2 ulp + gamma_{K-1} M per element, every channel beside a slice still the sentinel, every
case run twice with bit-identical results.

Paths reached (work items = pixels x channel groups; ew_grid caps a grid at 4096 x 256 of them):
    V = 1 by channel count   C = 12 in 16 bit, C = 6 in fp32                    V = 1 by alignment   the slice at channel 4 (fp32: 2) of 24
    vector form              C = 8, 16, 24, 32 dense and the SPPF slices        ACC                  acc_into= / accumulate=True
    second trip              more than 1,048,576 work items at V = 1 (sm.big_shape; the upsample forward counts OUTPUT pixels)
    k_multi_copy             the four vector pairs, the five scalar pairs, the < 8 tail, the unaligned (scalar) route, the
                             binary search over 1 / 2 / 37 jobs, scale 1, 1/8, 1/3
    k_pack_tiles             fp32 float4 loads and the scalar loads (16-bit sources, I k k % 4 != 0), vector and scalar
                             stores in both forms, partial 32 x 32 tiles, stride-2 parity classes"""
import time

import pytest
import torch
import torch.nn.functional as F

import strict_compare as sc
import strict_move as sm

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, HF = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]


def ops():
    from src.hipops import ops as o
    return o


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    t0 = time.time()
    yield
    print("\n" + sc.report() + "\n" + sm.report() + f"\n[strict_move] wall time of tests/test_gpu_move.py: {time.time() - t0:.1f} s")


def tid(d):
    return IDS[DTYPES.index(d)]


def sid(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


def place(t, ctot=None, off=0):
    """CPU (N, C, H, W) -> (whole NHWC buffer of ctot channels filled with the sentinel, its slice [off, off + C) holding t)"""
    n, c, h, w = t.shape
    buf = ops().new_nhwc(n, ctot or c, h, w, t.dtype, DEV)
    buf.fill_(sm.SENTINEL)
    view = buf[:, off:off + c]
    view.copy_(t.to(DEV))
    return buf, view


def layout(lay, c, dtype):
    """-> (channels of the underlying buffer, channel offset of the slice)"""
    if lay == "dense":
        return c, 0
    if lay == "unaligned":                                    # ld % V == 0, C % V == 0, the pointer 8 bytes past a 16-byte boundary
        return c + 8, 2 if dtype == F32 else 4
    return c + 8, 0                                           # "wide": aligned slice of a wider buffer


def twice(once):
    """run the case twice: every tensor it returns bit-identical; -> the first result"""
    a, b = once(), once()
    for k in a:
        assert torch.equal(sm.bits(a[k]), sm.bits(b[k])), f"{k}: two runs differ"
    return a


def cpu(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


# ------------------------------------------------------------------------------------------ pool
POOL_CASES = [(s, "dense") for s in sm.POOL_SHAPES] + [(sm.SLICE_SHAPE, "unaligned"), (sm.SPPF_SHAPE, "sppf"), ("big", "dense")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,lay", POOL_CASES, ids=[f"{sid(s)}-{l}" for s, l in POOL_CASES])
def test_maxpool5_forward_and_backward(shape, lay, dtype):
    o = ops()
    shape = sm.big_shape(dtype) if shape == "big" else shape
    n, c, h, w = shape
    x, dout, base = sm.grid(shape, 40, dtype), sm.smooth(shape, 41, dtype), sm.smooth(shape, 42, dtype)
    ctot, off = layout(lay, c, dtype)

    def once():
        if lay == "sppf":                                     # input slice 0, output slice 1 of one buffer; dout slice 1,
            obuf, xv = place(x, 4 * c, 0)                     # acc_into slice 0 of the gradient buffer
            ov = obuf[:, c:2 * c]
            gbuf, dv = place(dout, 4 * c, c)
            av = gbuf[:, :c]
            av.copy_(base.to(DEV))
        else:
            _, xv = place(x, ctot, off)
            obuf, ov = place(torch.zeros_like(x), ctot, off)
            _, dv = place(dout, ctot, off)
            gbuf, av = place(base, ctot, off)
        out, idx = o.maxpool5_fwd(xv, out=None if lay == "dense" else ov)
        dx = o.maxpool5_bwd(dv, idx)
        dxa = o.maxpool5_bwd(dv, idx, acc_into=av)
        assert dxa.data_ptr() == av.data_ptr() and tuple(idx.shape) == (n, h, w, c) and idx.dtype == torch.uint8
        return {"out": cpu(out), "idx": cpu(idx.permute(0, 3, 1, 2)), "dx": cpu(dx), "dxa": cpu(dxa), "obuf": cpu(obuf), "gbuf": cpu(gbuf)}

    r = twice(once)
    what = f"maxpool5 {shape} {lay} {tid(dtype)}"
    ridx = sm.check_pool_fwd(x, r["out"], r["idx"], what)
    sm.check_pool_bwd(dout, ridx, r["dx"], what + " bwd")
    sm.check_pool_bwd(dout, ridx, r["dxa"], what + " bwd acc_into", base)
    if lay == "sppf":
        sm.assert_guard(r["obuf"], 0, 2 * c, what + " forward")
        sm.assert_exact(r["obuf"][:, :c], x, what + " the input slice", "guard")
        sm.assert_guard(r["gbuf"], 0, 2 * c, what + " backward")
        sm.assert_exact(r["gbuf"][:, c:2 * c], dout, what + " the dout slice", "guard")
    elif lay != "dense":
        sm.assert_guard(r["obuf"], off, off + c, what + " forward")
        sm.assert_guard(r["gbuf"], off, off + c, what + " backward")


# ------------------------------------------------------------------------------------------ upsample
UP_CASES = [(s, "dense") for s in sm.UP_SHAPES] + [(sm.SLICE_SHAPE, "unaligned"), ("big", "dense")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,lay", UP_CASES, ids=[f"{sid(s)}-{l}" for s, l in UP_CASES])
def test_upsample2x_forward_and_backward(shape, lay, dtype):
    """big: the forward on a quarter of sm.big_shape (its OUTPUT has more than 1,048,576 work items), the backward onto
    sm.big_shape (its dx has)"""
    o = ops()
    if shape == "big":
        n, c, h2, w2 = sm.big_shape(dtype)
        shape, bshape = (n, c, h2 // 2, w2 // 2), (n, c, h2, w2)
    else:
        bshape = shape
    n, c, h, w = shape
    bn, bc, bh, bw = bshape
    x, dout, base = sm.grid(shape, 43, dtype), sm.smooth((bn, bc, 2 * bh, 2 * bw), 44, dtype), sm.smooth(bshape, 45, dtype)
    ctot, off = layout(lay, c, dtype)

    def once():
        _, xv = place(x, ctot, off)
        obuf, ov = place(torch.zeros(n, c, 2 * h, 2 * w, dtype=dtype), ctot, off)
        _, dv = place(dout, ctot, off)
        gbuf, av = place(base, ctot, off)
        up = o.upsample2x_fwd(xv, out=None if lay == "dense" else ov)
        dx = o.upsample2x_bwd(dv)
        dxa = o.upsample2x_bwd(dv, acc_into=av)
        assert dxa.data_ptr() == av.data_ptr()
        return {"up": cpu(up), "dx": cpu(dx), "dxa": cpu(dxa), "obuf": cpu(obuf), "gbuf": cpu(gbuf)}

    r = twice(once)
    what = f"upsample2x {shape} {lay} {tid(dtype)}"
    sm.check_up_fwd(x, r["up"], what)
    sm.check_up_bwd(dout, r["dx"], what + " bwd")
    sm.check_up_bwd(dout, r["dxa"], what + " bwd acc_into", base)
    if lay != "dense":
        sm.assert_guard(r["obuf"], off, off + c, what + " forward")
        sm.assert_guard(r["gbuf"], off, off + c, what + " backward")


# ------------------------------------------------------------------------------------------ copy_channels, add_n
COPY_CASES = [(s, v) for s in sm.COPY_SHAPES for v in ("dense", "slices")] + [("big", "dense")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,variant", COPY_CASES, ids=[f"{sid(s)}-{v}" for s, v in COPY_CASES])
def test_copy_channels_with_and_without_accumulate(shape, variant, dtype):
    """slices: the source an aligned slice of a wider buffer, the destination an unaligned slice (V = 1 by alignment)"""
    o = ops()
    shape = sm.big_shape(dtype) if shape == "big" else shape
    c = shape[1]
    src, dst = sm.smooth(shape, 46, dtype), sm.smooth(shape, 47, dtype)
    ls, ld = (("wide", "unaligned") if variant == "slices" else ("dense", "dense"))

    def once():
        res = {}
        for acc in (False, True):
            _, sv = place(src, *layout(ls, c, dtype))
            dbuf, dvw = place(dst, *layout(ld, c, dtype))
            o.copy_channels(sv, dvw, acc)
            res[f"d{int(acc)}"], res[f"buf{int(acc)}"] = cpu(dvw), cpu(dbuf)
        return res

    r = twice(once)
    for acc in (False, True):
        what = f"copy_channels {shape} {variant} acc={acc} {tid(dtype)}"
        sm.check_copy(src, dst, r[f"d{int(acc)}"], what, acc)
        if variant == "slices":
            off = layout(ld, c, dtype)[1]
            sm.assert_guard(r[f"buf{int(acc)}"], off, off + c, what)


ADD_CASES = [(s, v, k) for s in sm.COPY_SHAPES for v in ("dense", "slices") for k in (2, 3, 4)] + [("big", "dense", 3)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,variant,k", ADD_CASES, ids=[f"{sid(s)}-{v}-k{k}" for s, v, k in ADD_CASES])
def test_add_n_with_cancellation(shape, variant, k, dtype):
    """slices: the sources dense / an aligned slice / an unaligned slice / dense, out= an aligned slice of a wider buffer;
    channel 3 holds two large values of opposite sign next to small ones"""
    o = ops()
    shape = sm.big_shape(dtype) if shape == "big" else shape
    c = shape[1]
    xs = sm.cancel([sm.smooth(shape, 50 + i, dtype) for i in range(k)])
    lays = ["dense", "wide", "unaligned", "dense"] if variant == "slices" else ["dense"] * 4

    def once():
        vs = [place(x, *layout(l, c, dtype))[1] for x, l in zip(xs, lays)]
        fresh = o.add_n(vs)
        obuf, ov = place(torch.zeros_like(xs[0]), c + 16, 8)
        into = o.add_n(vs, out=ov)
        assert into.data_ptr() == ov.data_ptr()
        return {"fresh": cpu(fresh), "into": cpu(into), "obuf": cpu(obuf)}

    r = twice(once)
    what = f"add_n {k} {shape} {variant} {tid(dtype)}"
    sm.check_add(xs, r["fresh"], what)
    sm.check_add(xs, r["into"], what + " into a slice")
    sm.assert_guard(r["obuf"], 8, 8 + c, what)


# ------------------------------------------------------------------------------------------ transposes
PAIRS = [(s, d) for s in DTYPES for d in DTYPES]


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{tid(s)}-to-{tid(d)}" for s, d in PAIRS])
@pytest.mark.parametrize("shape", [(2, 37, 9, 11), (1, 1, 1, 1)], ids=sid)
def test_transposes_store_the_correctly_rounded_value(shape, src, dst):
    """to_nhwc and head_pack at every source / destination pair (k_ncm_to_nhwc, k_nhwc_to_ncm); head_unpack has one dtype by
    its signature and runs where source and destination agree"""
    o = ops()
    n, c, h, w = shape
    x = sm.edge_vals(shape, 7, src)

    def once():
        y = o.to_nhwc(x.to(DEV), dst)
        assert o.is_nhwc(y) and y.dtype == dst
        xn = o.to_nhwc(x.to(DEV), src)
        preds = torch.full((n, c + 13, h * w + 30), sm.SENTINEL, dtype=dst, device=DEV)
        o.head_pack(xn, preds, 5, 20)
        res = {"y": cpu(y), "preds": cpu(preds)}
        if src == dst:
            res["back"] = cpu(o.head_unpack(preds, 5, c, 20, h, w))
        return res

    r = twice(once)
    what = f"{shape} {tid(src)} -> {tid(dst)}"
    sm.check_cast(x, r["y"], "to_nhwc " + what)
    want = torch.full((n, c + 13, h * w + 30), sm.SENTINEL, dtype=dst)
    want[:, 5:5 + c, 20:20 + h * w] = sm.cast_ref(x, dst).reshape(n, c, h * w)
    sm.assert_exact(r["preds"], want, "head_pack " + what)
    if src == dst:
        sm.assert_exact(r["back"], x, "head_unpack " + what)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_head_group_with_an_odd_branch_takes_the_two_byte_form(dtype):
    """M = 24 and every channel count a multiple of 8, but HW = 15 and m_off = 15: no 16-byte form; still exact both ways"""
    o = ops()
    n = 2
    maps, c_offs, m_offs = [(16, 3, 5), (16, 3, 3), (8, 3, 3)], [3, 3, 19], [0, 15, 15]
    xs = [sm.edge_vals((n, c, h, w), 80 + i, dtype) for i, (c, h, w) in enumerate(maps)]

    def once():
        br = [place(x)[1] for x in xs]
        preds = torch.full((n, 30, 24), sm.SENTINEL, dtype=dtype, device=DEV)
        o.head_group(br, preds, c_offs, m_offs, True)
        outs = [place(torch.zeros_like(x), x.shape[1] + 8, 0) for x in xs]
        o.head_group([v for _, v in outs], preds, c_offs, m_offs, False)
        res = {"preds": cpu(preds)}
        for i, (b, _) in enumerate(outs):
            res[f"b{i}"] = cpu(b)
        return res

    r = twice(once)
    want = torch.full((n, 30, 24), sm.SENTINEL, dtype=dtype)
    for x, co, mo in zip(xs, c_offs, m_offs):
        c, hw = x.shape[1], x.shape[2] * x.shape[3]
        want[:, co:co + c, mo:mo + hw] = x.reshape(n, c, hw)
    sm.assert_exact(r["preds"], want, f"head_group pack {tid(dtype)}")
    for i, x in enumerate(xs):
        sm.assert_exact(r[f"b{i}"][:, :x.shape[1]], x, f"head_group unpack branch {i} {tid(dtype)}")
        sm.assert_guard(r[f"b{i}"], 0, x.shape[1], f"head_group unpack branch {i} {tid(dtype)}")


# ------------------------------------------------------------------------------------------ bucket_copy
SIZES = [1, 7, 8, 9, 4095, 4096, 4097, 8195, 5000]
JOBS = {1: [8195], 2: [4097, 5000], 37: [SIZES[i % 9] for i in range(37)]}


def bucket_case(src_dt, dst_dt, sizes, scale):
    """the job table as GradBuckets._plan builds it, from explicit (src, dst) pairs: slices of one flat source and one flat
    destination buffer, every start 32-byte aligned except job 3's source and job 5's destination (one element past: the
    scalar route); the gaps of the destination hold the sentinel"""
    from src.hipops import lib
    o = ops()
    so, do, s_end, d_end = [], [], 0, 0
    for i, n in enumerate(sizes):
        so.append(s_end + (1 if i == 3 or len(sizes) == 1 else 0))
        do.append(d_end + (1 if i == 5 else 0))
        s_end = -(-(so[-1] + n + 3) // 16) * 16
        d_end = -(-(do[-1] + n + 9) // 16) * 16
    src = sm.edge_vals((s_end,), 90, src_dt)

    def once():
        s_dev = src.to(DEV)
        d_dev = torch.full((d_end,), sm.SENTINEL, dtype=dst_dt, device=DEV)
        jb = lib.query("yolo_copy_job_bytes")
        host = torch.zeros(len(sizes) * jb, dtype=torch.uint8)
        srcs, dsts = [], []
        for i, n in enumerate(sizes):
            srcs.append(s_dev[so[i]:so[i] + n])
            dsts.append(d_dev[do[i]:do[i] + n])
            lib.call("yolo_copy_job_fill", host.data_ptr(), i, srcs[-1].data_ptr(), o.dt(src_dt), dsts[-1].data_ptr(), o.dt(dst_dt), n)
        nchunks = lib.query("yolo_copy_jobs_finalize", host.data_ptr(), len(sizes))       # before the upload: it writes cstart
        plan = dict(dev=host.to(DEV), njobs=len(sizes), nchunks=nchunks, srcs=srcs, dsts=dsts)
        assert plan["nchunks"] == sum(max(1, -(-n // 4096)) for n in sizes)
        o.bucket_copy(plan, scale)
        return {"dst": cpu(d_dev), "src": cpu(s_dev)}

    r = twice(once)
    want = torch.full((d_end,), sm.SENTINEL, dtype=dst_dt)
    for i, n in enumerate(sizes):
        want[do[i]:do[i] + n] = sm.cast_ref(src[so[i]:so[i] + n], dst_dt, scale)
    what = f"bucket_copy {tid(src_dt)} -> {tid(dst_dt)} x {scale:g}, {len(sizes)} jobs"
    sm.assert_exact(r["dst"], want, what)
    sm.assert_exact(r["src"], src, what + ": the source", "guard")


@pytest.mark.parametrize("scale", [1.0, 0.125, 1.0 / 3.0], ids=["x1", "x0.125", "x1over3"])
@pytest.mark.parametrize("njobs", [1, 2, 37])
@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{tid(s)}-to-{tid(d)}" for s, d in PAIRS])
def test_bucket_copy_every_pair_size_and_route(src, dst, njobs, scale):
    """sizes 1, 7, 8, 9 (the < 8 tail alone, none, one element), 4095 / 4096 / 4097 (the chunk edge), 8195, 5000; one job
    (unaligned source: the scalar route at every pair), two, and 37 (the binary search, two unaligned jobs among them)"""
    bucket_case(src, dst, JOBS[njobs], scale)


# ------------------------------------------------------------------------------------------ the batched weight pack
CONVS = [(16, 16, 1, 1), (40, 24, 3, 1), (33, 20, 3, 2), (64, 32, 3, 2), (130, 70, 1, 1), (24, 6, 3, 1)]      # O, I, k, stride


@pytest.mark.parametrize("out_dt", [BF, HF], ids=IDS[1:])
@pytest.mark.parametrize("w_dt", DTYPES, ids=IDS)
def test_weight_pack_plan_equals_the_per_layer_pack(w_dt, out_dt):
    """partial 32 x 32 tiles in both directions, O or I not a multiple of 8 (scalar stores), I k k not a multiple of 4 and
    16-bit sources (scalar loads), stride-2 parity classes; one plan for all six convs (the search over its jobs)"""
    o = ops()
    g = torch.Generator().manual_seed(11)
    ws = [(torch.randn(oc, ic, k, k, generator=g) * 0.5).to(w_dt).to(DEV) for oc, ic, k, s in CONVS]
    convs = [(w, k, s) for w, (_, _, k, s) in zip(ws, CONVS)]
    assert o.ACTIVE_PACK_PLAN is None
    plan = o.WeightPackPlan(convs, out_dt)
    plan.run()
    first = cpu(plan.flat).clone()
    plan.run()
    assert torch.equal(sm.bits(first), sm.bits(cpu(plan.flat))), "two runs differ"
    seen = 0
    for (w, k, s), shp in zip(convs, CONVS):
        for mode in (0, 1):
            view = plan.lookup(w, mode, out_dt)
            assert view is not None
            ref = o.pack_weights(w, k, s, mode, out_dt)
            assert ref.data_ptr() != view.data_ptr()
            sm.assert_exact(view, ref, f"pack {shp} mode {mode} {tid(w_dt)} -> {tid(out_dt)}", "pack")
            seen += view.numel()
    assert seen == plan.total


# ------------------------------------------------------------------------------------------ SPPF's backward as the model runs it
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 16, 12, 12), (2, 8, 3, 4)], ids=sid)
def test_sppf_backward_chain(shape, dtype):
    """fan2 / MaxPool5 with out= slices of one 4c-wide buffer / stash / CatInto exactly as SPPF.forward (without the two
    convs), a random gradient for the concat: the gradient of the first map against float64 autograd of three chained
    F.max_pool2d and a cat, inside the bound propagated stage by stage (strict_move.chain_ref)"""
    from src.hipops import functions as F_
    o = ops()
    n, c, h, w = shape
    x, g = sm.grid(shape, 60, dtype), sm.smooth((n, 4 * c, h, w), 61, dtype)

    def once():
        buf = o.new_nhwc(n, 4 * c, h, w, dtype, DEV)
        buf.fill_(sm.SENTINEL)
        buf[:, :c].copy_(x.to(DEV))
        x0 = buf[:, :c].detach().requires_grad_(True)
        xa, l0 = F_.fan2(x0)
        y1, l1 = F_.fan2(F_.MaxPool5.apply(xa, buf[:, c:2 * c], l0))
        y2, l2 = F_.fan2(F_.MaxPool5.apply(y1, buf[:, 2 * c:3 * c], l1))
        y3 = F_.MaxPool5.apply(y2, buf[:, 3 * c:], l2)
        cat = F_.CatInto.apply(buf, F_.stash(xa, l0), F_.stash(y1, l1), F_.stash(y2, l2), y3)
        gd = place(g)[0]
        cat.backward(gd)
        assert l0.dres is None and l1.dres is None and l2.dres is None
        return {"dx": cpu(x0.grad), "fwd": cpu(buf)}

    r = twice(once)
    what = f"SPPF chain {shape} {tid(dtype)}"
    _, ref = sm.check_chain(x, g, r["dx"], what)
    sm.assert_exact(r["fwd"], torch.cat([x.double()] + list(ref["y"]), 1).to(dtype), what + " forward", "pool_out")
    xd = x.double().requires_grad_(True)                       # the reference itself is float64 autograd
    p1 = F.max_pool2d(xd, 5, 1, 2)
    p2 = F.max_pool2d(p1, 5, 1, 2)
    (want,) = torch.autograd.grad(torch.cat([xd, p1, p2, F.max_pool2d(p2, 5, 1, 2)], 1), xd, g.double())
    fin = torch.isfinite(want)
    assert torch.equal(fin, torch.isfinite(ref["v0"])) and torch.equal(torch.isnan(want), torch.isnan(ref["v0"]))
    assert float((ref["v0"] - want)[fin].abs().max()) <= 1e-12 * float(want[fin].abs().max())
