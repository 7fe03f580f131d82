"""The case tables of tests/test_gpu_nonfinite.py, with the poison positions and the dependency sets of every case -- all of it
CPU-only (float64 references on indicator tensors, strict_nonfinite.py), so that tests/test_strict_nonfinite_cpu.py can show
without a GPU that every case lies inside the helper's two refusal conditions (dep neither empty nor more than half of the
output; no exact zero among the multiplying operands).

Shapes: the forced-variant tables of tests/test_gpu_conv_variants.py (every gather width in both staging modes, every ring
tile at every depth, every halo and rows variant, the stride-2 patch data gradient of csrc/conv_up2.hip, every weight-gradient
tile) on the 7 x 11 / 9 x 20 maps of its statistics test -- a partial last pixel tile and, with 72 / 200 destination channels,
a partial last channel tile; 96 source channels: a partial last 64-deep K-step.  Depthwise: a subset of the CASES of
tests/test_gpu_dw_rows.py plus the 12-channel map of the generic kernel.  BatchNorm: SHAPES of tests/test_gpu_bn.py.
Batches hold three distinct images (strict_compare.image_pattern(3))."""
import torch

import strict_nonfinite as sn

N = 3
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


def positions(n, c, h, w, tail, chans=None, interior=False):
    """Poison positions of an (n, c, h, w) tensor: the first element; the last channel of the last pixel of the last image;
    a corner pixel of the middle image (padding taps); the last row of image 0 and the first row of image 1 (the boundary
    that flattened or clamped pixel indices confuse); a channel of the partial last K-step / channel tile (`tail`) at the left
    edge.  chans: only channels 0, tail and c - 1 (the weight-gradient and per-channel cases, whose dep is whole channels).
    interior (the weight gradient's x and dy): each of the three channels also gets the 2 x 2 block of pixels in the middle of
    the map (both parities of a stride-2 conv), where every tap of the kernel meets a pixel of the other operand.  'NaN in one
    x channel means exactly dw[:, ci] for the taps that exist, in one dy channel exactly dw[co]' then holds as whole rows for
    every sound way of forming the sums: a tap whose only poisoned terms pair the NaN with something that is not there (the
    padding of x; an output pixel past the last row, which a tile tail reads as a zero record) is 0 x NaN for a kernel that
    masks by zero records and an empty sum for one that skips -- inside a row that is poisoned either way.  The positions are
    chosen so that the question does not arise ('NaN / Inf propagation').
    Duplicates (maps of one row or column) are dropped; "inf" alternates +inf / -inf in this order."""
    m = min(1, n - 1)
    mid, low = (tail, 0) if chans else (c // 2, 1 % c)
    cand = [(0, 0, 0, 0), (n - 1, c - 1, h - 1, w - 1), (m, mid, 0, w - 1), (0, tail, h - 1, w // 2), (m, low, 0, w // 2),
            (n - 1, tail, h // 2, 0)]
    if interior:
        for img, ch in ((m, 0), (0, c - 1), (n - 1, tail)):
            cand += [(img, ch, hh, ww) for hh in (max(h // 2 - 1, 0), h // 2) for ww in (max(w // 2 - 1, 0), w // 2)]
    return list(dict.fromkeys(cand))


def rnd(shape, seed, scale=1.0, dtype=BF):
    """seeded values of `dtype` without an exact zero (strict_nonfinite.fix_zeros)"""
    g = torch.Generator().manual_seed(seed)
    return sn.fix_zeros((torch.randn(*shape, generator=g) * scale).to(dtype))


def out_hw(h, w, k, s):
    return (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1


# --------------------------------------------------------------------------------------------------- dense convolution
def ring_plan(bm, bn):
    return 3000 + (500 if bm == 64 else 0) + bn


RING_TILES = [(64, 128, 128), (64, 128, 64), (64, 64, 128), (64, 64, 64), (64, 128, 32),
              (32, 128, 128), (32, 128, 64), (32, 64, 128), (32, 64, 64)]          # (bk, bm, bn) of tests/test_gpu_conv_variants.py


def _dense(id_, tune, plan, family, cin, cout, h, w, k, s, **kw):
    d = dict(id=id_, tune=tune, plan=plan, family=family, cin=cin, cout=cout, h=h, w=w, k=k, s=s, algo=0, stats=True, fused=True,
             dgrad=True, dtypes=(BF, HF))
    d.update(kw)
    return d


DENSE = []
for _bn in (32, 64, 128):
    for _dma in (0, 1):
        for _sh in ((64, 72, 3, 1), (96, 200, 1, 1), (64, 64, 3, 2)):
            DENSE.append(_dense(f"gather-bn{_bn}-{'dma' if _dma else 'registers'}-{_sh[0]}x{_sh[1]}k{_sh[2]}s{_sh[3]}",
                                (_bn, -1, 0, _dma, 0, 0, 0, 0), 1000 + _bn, "gather", _sh[0], _sh[1], 7, 11, _sh[2], _sh[3]))
for _bk, _bm, _bn in RING_TILES:
    for _nst in (2, 3, 4):
        # 96 source channels: one full and one partial 64-deep K-step; 1x1 on 200 and 3x3 on 72 destination channels in turn
        _sh = (96, 72, 3, 1) if (_nst + _bn // 32) % 2 else (96, 200, 1, 1)
        DENSE.append(_dense(f"ring-bk{_bk}-{_bm}x{_bn}-depth{_nst}-k{_sh[2]}", (_bn, -1, 0, -1, 1, _bm, _nst, _bk), ring_plan(_bm, _bn), "ring",
                            _sh[0], _sh[1], 7, 11, _sh[2], _sh[3], dtypes=(BF, HF) if _nst == 3 else ((BF,) if _nst == 2 else (HF,))))
for _v in (1, 2, 3, 4):
    DENSE.append(_dense(f"halo-{_v}", (0, -1, _v, -1, -1, 0, 0, 0), 2000 + _v, "halo", 96 if _v % 2 else 64, 72, 7, 11, 3, 1))
for _f, _plan, _cin, _cout, _h, _w in ((6, 4001, 64, 72, 9, 20), (7, 4002, 96, 200, 9, 20), (8, 4003, 64, 72, 9, 20), (12, 4004, 64, 72, 9, 20),
                                       (14, 4006, 64, 72, 7, 11), (16, 4007, 16, 24, 7, 11)):
    DENSE.append(_dense(f"rows-{_f}", (0, -1, _f, -1, -1, 0, 0, 0), _plan, "rows", _cin, _cout, _h, _w, 3, 1))
AUTO = (0, -1, -1, -1, -1, 0, 0, 0)
# the stride-2 data gradient of csrc/conv_up2.hip (plan of mode 1: 5016 / 5008), reached by the launcher's own choice on
# an even map; the dy grid 7 x 11 is no multiple of its 8- / 16-row and 16-column tiles
DENSE.append(_dense("patch-16", AUTO, None, "auto", 32, 64, 14, 22, 3, 2, dplan=5016, stats=False, fused=False))
DENSE.append(_dense("patch-8", AUTO, None, "auto", 72, 96, 14, 22, 3, 2, dplan=5008, stats=False, fused=False))
# the generic VALU kernels (12 source channels: no MFMA kernel takes them; and forced by algo 1) and the fp32 kernels
DENSE.append(_dense("generic-cin12", AUTO, 0, "generic", 12, 16, 7, 11, 3, 1, stats=False, fused=False, dgrad=False, dtypes=(BF,)))
DENSE.append(_dense("generic-forced", AUTO, None, "generic", 16, 24, 7, 11, 3, 2, algo=1, stats=False, fused=False))
DENSE.append(_dense("fp32", AUTO, 0, "fp32", 16, 24, 7, 11, 3, 1, stats=False, fused=False, dtypes=(F32,)))
DENSE.append(_dense("fp32-1x1", AUTO, 0, "fp32", 24, 40, 7, 11, 1, 1, stats=False, fused=False, dtypes=(F32,)))


def dense_inputs(case, dtype):
    cin, cout, h, w, k, s = (case[key] for key in ("cin", "cout", "h", "w", "k", "s"))
    oh, ow = out_hw(h, w, k, s)
    seed = sum(map(ord, case["id"]))
    return {"x": rnd((N, cin, h, w), seed + 1, dtype=dtype), "w": rnd((cout, cin, k, k), seed + 2, (cin * k * k) ** -0.5, dtype),
            "dy": rnd((N, cout, oh, ow), seed + 3, dtype=dtype), "base": rnd((N, cin, h, w), seed + 4, dtype=dtype),
            "acc2": rnd((N, cin, h, w), seed + 5, dtype=dtype), "res": rnd((N, cout, oh, ow), seed + 7, dtype=dtype),
            "bias": rnd((cout,), seed + 6, 0.5, F32)}


def dense_plan(case):
    """-> positions and dependency sets of every launch of a dense case (float64 references on indicators)"""
    cin, cout, h, w, k, s = (case[key] for key in ("cin", "cout", "h", "w", "k", "s"))
    oh, ow = out_hw(h, w, k, s)
    xs, ys, ws = (N, cin, h, w), (N, cout, oh, ow), (cout, cin, k, k)
    p = {"x": positions(N, cin, h, w, cin - 3), "dy": positions(N, cout, oh, ow, cout - 3),
         "w": [(cout - 3, cin - 3, k // 2, k // 2)],
         "base": [(N - 1, cin // 3, h // 2, w - 1)], "acc2": [(0, cin - 1, 0, w // 2)], "res": [(N - 1, cout // 3, oh // 2, ow - 1)],
         "x_w": positions(N, cin, h, w, cin - 3, chans=True, interior=True), "dy_w": positions(N, cout, oh, ow, cout - 3, chans=True, interior=True)}
    d = {"fwd": sn.conv_dep(sn.indicator(xs, p["x"]), ws, k, s), "fwd_w": sn.conv_dep_w(xs, sn.indicator(ws, p["w"]), k, s)}
    d["stats_w"] = d["fwd_w"].any(0).any(-1).any(-1).view(1, cout).expand(2, cout).clone()
    d["fused"] = d["fwd"] | (sn.indicator(ys, p["res"]) > 0)
    d["dgrad"] = sn.dgrad_dep(sn.indicator(ys, p["dy"]), ws, xs, k, s)
    d["dgrad_acc"] = d["dgrad"] | (sn.indicator(xs, p["base"]) > 0)
    d["dgrad_acc2"] = d["dgrad_acc"] | (sn.indicator(xs, p["acc2"]) > 0)
    d["wgrad_x"] = sn.wgrad_dep(sn.indicator(xs, p["x_w"]), ys, ws, k, s)
    d["wgrad_dy"] = sn.wgrad_dep(xs, sn.indicator(ys, p["dy_w"]), ws, k, s)
    # the same without the interior pixels: the pixel-exact set, decidable wherever a row is not poisoned at all
    p["x_edge"] = positions(N, cin, h, w, cin - 3, chans=True)
    d["wgrad_x_edge"] = sn.wgrad_dep(sn.indicator(xs, p["x_edge"]), ys, ws, k, s)
    return p, d


# every forced weight-gradient tile of tests/test_gpu_conv_variants.py: (to, ti, pf, cin, cout, k, s); + the atomics path (algo 3)
WGRAD = [(to, ti, pf, 72, 88, 3, s) for to in (1, 2) for ti in (1, 2) for pf, s in ((1, 1), (4, 2), (4, 1))] + \
        [(to, ti, 1 if (to + ti) % 2 else 4, 136, 120, 1, 1) for to in (1, 2, 3, 4) for ti in (1, 2, 3, 4)]
WGRAD_ATOMICS = [(72, 88, 3, 1), (72, 88, 3, 2), (136, 120, 1, 1)]


def wgrad_case(cin, cout, k, s):
    return _dense(f"wgrad-{cin}x{cout}k{k}s{s}", AUTO, None, "wgrad", cin, cout, 7, 11, k, s)


# the stem: 3 -> 32 channels on an 18 x 22 image (tests/test_gpu_conv_variants.py's statistics case)
STEM = dict(cout=32, h=18, w=22)


def stem_plan():
    cout, h, w = STEM["cout"], STEM["h"], STEM["w"]
    oh, ow = out_hw(h, w, 3, 2)
    xs, ys, ws = (N, 3, h, w), (N, cout, oh, ow), (cout, 3, 3, 3)
    p = {"img": [(0, 0, 0, 0), (N - 1, 2, h - 1, w - 1), (1, 1, 0, w - 1), (0, 1, h - 1, w // 2), (1, 0, 0, w // 2)],
         "img_w": [(0, 1, 0, 0), (N - 1, 1, h - 1, w - 1), (1, 1, 0, w // 2), (0, 1, h - 1, w // 2)] +
                  [(1, 1, hh, ww) for hh in (h // 2 - 1, h // 2) for ww in (w // 2 - 1, w // 2)],       # both parities: every tap (positions())
         "dy_w": positions(N, cout, oh, ow, cout - 3, chans=True, interior=True)}
    d = {"fwd": sn.conv_dep(sn.indicator(xs, p["img"]), ws, 3, 2),
         "wgrad_img": sn.wgrad_dep(sn.indicator(xs, p["img_w"]), ys, ws, 3, 2),
         "wgrad_dy": sn.wgrad_dep(xs, sn.indicator(ys, p["dy_w"]), ws, 3, 2)}
    d["chan_dy"] = d["wgrad_dy"].flatten(1).any(1)
    return p, d


# --------------------------------------------------------------------------------------------------- depthwise
# (C, H, W, x is a slice of a wider buffer, dy is one): H = 1, 2, 3; a partial band (7); W = 1 and 21; C = 8, 24, 2056; 12
DW = [(16, 1, 6, 0, 1), (16, 2, 6, 1, 0), (16, 3, 6, 0, 1), (16, 7, 6, 1, 0), (16, 5, 1, 1, 0), (128, 5, 21, 1, 0), (8, 5, 6, 1, 0),
      (24, 6, 7, 0, 1), (2056, 3, 5, 0, 1)]
DW_GENERIC = (12, 5, 6, 0, 1)


def dw_inputs(c, h, w, dtype):
    return {"x": rnd((N, c, h, w), 50 + c + h, dtype=dtype), "dy": rnd((N, c, h, w), 51 + c + h, dtype=dtype),
            "w9": rnd((c, 9), 52 + c, 0.3, F32), "bias": rnd((c,), 53 + c, 0.5, F32), "base": rnd((N, c, h, w), 54 + c + h, dtype=dtype)}


def dw_plan(c, h, w):
    """`taps`: the (3, 3) taps that meet an output pixel at all -- on a map of one row or one column the others are an empty sum
    for a kernel that skips the padding and 0 x dy for one that reads it as a zero record (see positions()); the weight
    gradient is compared on the taps that exist"""
    xs, ws = (N, c, h, w), (c, 1, 3, 3)
    p = {"x": positions(N, c, h, w, c - 3, chans=True, interior=True), "base": [(N - 1, c // 3, h // 2, w - 1)]}
    p["dy"] = p["x"]
    ind = ind_dy = sn.indicator(xs, p["x"])
    taps = sn.wgrad_dep((N, 1, h, w), (N, 1, h, w), (1, 1, 3, 3), 3, 1)[0, 0]
    d = {"fwd": sn.conv_dep(ind, ws, 3, 1, groups=c), "dgrad": sn.dgrad_dep(ind_dy, ws, xs, 3, 1, groups=c), "taps": taps,
         "wgrad_x": sn.wgrad_dep(ind, xs, ws, 3, 1, groups=c)[:, :, taps], "wgrad_dy": sn.wgrad_dep(xs, ind_dy, ws, 3, 1, groups=c)[:, :, taps]}
    d["dgrad_acc"] = d["dgrad"] | (sn.indicator(xs, p["base"]) > 0)
    d["stats"] = d["fwd"].any(0).any(-1).any(-1).view(1, c).expand(2, c).clone()
    return p, d


# --------------------------------------------------------------------------------------------------- BatchNorm
# (n, c, h, w, pad, residual) of tests/test_gpu_bn.py's SHAPES: one element per lane; 16-byte packets; a slice 2 channels in;
# a partly filled last channel group with residual; a second blockIdx.y group of one packet
BN = [(3, 6, 11, 13, 0, True), (3, 24, 11, 13, 16, False), (3, 24, 11, 13, 4, False), (3, 264, 11, 13, 0, True), (2, 2056, 3, 5, 0, False)]


def bn_plan(n, c, h, w):
    """one element of channel c - 3 -> the whole channel: (position, per-channel mask (c,), per-element mask (n, c, h, w))"""
    ch = c - 3
    pos = [(n - 1, ch, h // 2, w - 1)]
    chan = torch.zeros(c, dtype=torch.bool)
    chan[ch] = True
    return pos, chan, chan.view(1, c, 1, 1).expand(n, c, h, w).clone()


# --------------------------------------------------------------------------------------------------- attention
# (route, dtype, heads, dk, dh, tokens): every route tests/test_gpu_kernels.py selects, 2 images x 2 heads, 36 tokens (a
# partial last 16-row and 64-column block) and 449 (one past the one-image kernels' 448)
ATTN = [("fused", BF, 2, 32, 64, 36), ("fused", HF, 2, 32, 64, 36), ("gemm", BF, 2, 16, 32, 36), ("gemm", HF, 2, 16, 32, 36),
        ("gemm", BF, 2, 32, 64, 449), ("fp32", F32, 2, 32, 64, 36)]
ATTN_NOGRAD = [("fused", BF, 2, 32, 64, 36), ("fused", HF, 2, 32, 64, 36), ("long", BF, 2, 32, 64, 449), ("long", HF, 2, 32, 64, 449)]
ATTN_N = 2


def attn_plan(heads, t):
    """(problem = image * heads + head, token) of the poisoned rows: the last token (partial row block) of the first image's
    last head for q and dO; a middle token of the second image's first head for k; the first token of that problem for v"""
    return {"q": (heads - 1, t - 1), "k": (heads, t // 2), "v": (heads, 0, 3), "do": (heads - 1, t - 1, 5), "dvp": (ATTN_N * heads - 1, 1, 7)}


def attn_channel(which, head, comp, heads, dk, dh):
    """channel of component `comp` of q / k / v of `head` in the (N, heads * (2 dk + dh), H, W) tensor (strict_attention.split_qkv)"""
    return head * (2 * dk + dh) + {"q": 0, "k": dk, "v": 2 * dk}[which] + comp


def all_dep_masks():
    """(name, dep, multiplying operands) of every case above, for the CPU module's sweep of the refusal conditions"""
    for case in DENSE:
        p, d = dense_plan(case)
        for dtype in case["dtypes"]:
            inp = dense_inputs(case, dtype)
            yield f"{case['id']} {str(dtype)[6:]}", d, {"w": inp["w"], "x": inp["x"], "dy": inp["dy"]}
    for cin, cout, k, s in sorted({c[3:] for c in WGRAD} | set(WGRAD_ATOMICS)):
        case = wgrad_case(cin, cout, k, s)
        p, d = dense_plan(case)
        inp = dense_inputs(case, BF)
        yield case["id"], {key: d[key] for key in ("wgrad_x", "wgrad_dy")}, {"x": inp["x"], "dy": inp["dy"]}
    yield "stem", stem_plan()[1], {}
    for c, h, w, _, _ in DW + [DW_GENERIC]:
        inp = dw_inputs(c, h, w, HF)
        yield f"dw {c}x{h}x{w}", {key: m for key, m in dw_plan(c, h, w)[1].items() if key != "taps"}, {"w9": inp["w9"], "x": inp["x"], "dy": inp["dy"]}
    for n, c, h, w, _, _ in BN:
        _, chan, full = bn_plan(n, c, h, w)
        yield f"bn {n}x{c}x{h}x{w}", {"channel": chan, "elements": full}, {}
    for route, dtype, heads, dk, dh, t in ATTN + ATTN_NOGRAD:
        r = attn_plan(heads, t)
        b = ATTN_N * heads
        yield f"attn {route} T={t} q", sn.attention_dep(b, t, dk, dh, q_rows=[r["q"]]), {}
        yield f"attn {route} T={t} k", sn.attention_dep(b, t, dk, dh, k_rows=[r["k"]]), {}
        yield f"attn {route} T={t} v", {key: m for key, m in sn.attention_dep(b, t, dk, dh, v_elems=[r["v"]]).items() if key not in ("lse", "dv")}, {}
        yield f"attn {route} T={t} dO", {key: m for key, m in sn.attention_dep(b, t, dk, dh, do_elems=[r["do"]], dvp_elems=[r["dvp"]]).items()
                                         if key not in ("lse", "o")}, {}
