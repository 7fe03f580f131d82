// Which kernel a dense forward / data-gradient convolution takes: the tune overrides, conv_select -- the ONE place that
// asks the families in order and holds the measured thresholds -- and the entry points, which call it and switch on its
// answer.  yolo_conv2d_plan reports the same answer, so "the plan says X" and "the launch takes X" cannot drift apart.
// Host code only: the kernels live in conv_generic / conv_f32 / conv_mfma / conv_halo / conv_ring / conv_rows / conv_up2.hip.
#include <cstdio>
#include <cstdlib>
#include "conv_host.h"

ConvTune& conv_tune() {
    static ConvTune t = [] {
        ConvTune v{0, -1, -1, -1, -1, 0, 0, 0};
        if (const char* e = getenv("YOLO_CONV_TUNE"))
            sscanf(e, "%d,%d,%d,%d,%d,%d,%d,%d", &v.bn, &v.tap_inner, &v.halo, &v.dma, &v.ring, &v.bm, &v.nst, &v.bk);
        return v;
    }();
    return t;
}

extern "C" int yolo_conv_tune_set(int bn, int tap_inner, int halo, int dma, int ring, int bm, int nst, int bk) {
    ConvTune& t = conv_tune();
    t.bn = bn; t.tap_inner = tap_inner; t.halo = halo; t.dma = dma; t.ring = ring; t.bm = bm; t.nst = nst; t.bk = bk;
    return YOLO_OK;
}

namespace {

// The third tune field ("halo") steers the halo kernel, the row-block kernel and the stride-2 patch kernel.  Its values
// (tuning runs, A/B runs and the variant-forcing parity tests; every value not listed acts like 15):
//    < 0   everything automatic (the default)
//      0   halo and rows off: the gather / ring kernels only
//   1..4   that halo variant wherever the halo kernel can run; rows off
//      5   rows by its measured defaults (as automatic); halo automatic
//   6 / 7 / 8 / 12   rows variant 1 / 2 (1 up to 64 destination channels) / 3 / 4 on maps that take its full-row blocks
//      9   rows off, everything else automatic
//     14   rows variant 6 (16-pixel-wide blocks x 64 channels) wherever it can run
//     15   rows in its full-row form only: the 16-pixel-wide forms off
//     16   rows variant 7 (16-pixel-wide blocks x 32 channels) on narrow layers
// From 6 up, whatever the value does not force stays automatic, except that rows' 16-pixel-wide forms are off by default.
// 0..4, like ring > 0, mean "a test is forcing another kernel": the patch kernel then stays out of its way.
struct ConvForce {
    int halo;                   // -1 automatic, 0 never, 1..4 this variant
    bool rows_off;              // never the row-block kernel
    bool rows_wide16_auto;      // its 16-pixel-wide forms (variants 6, 7) by their measured defaults
    int rows;                   // 0, or the forced rows variant: 1..4 full-row forms, 6, 7
    bool up2_off;               // never the patch kernel (also YOLO_DGRAD2_PATCH=0: A/B runs against the gather ring)
};
ConvForce conv_force() {
    static const int patch_env = [] { const char* e = getenv("YOLO_DGRAD2_PATCH"); return e ? atoi(e) : 1; }();
    const ConvTune& tu = conv_tune();
    const int v = tu.halo;
    const bool other = v >= 0 && v <= 4;
    ConvForce f;
    f.halo = other ? v : -1;
    f.rows_off = other || v == 9;
    f.rows_wide16_auto = v < 0 || v == 5;
    f.rows = v == 6 ? 1 : v == 7 ? 2 : v == 8 ? 3 : v == 12 ? 4 : v == 14 ? 6 : v == 16 ? 7 : 0;
    f.up2_off = other || tu.ring > 0 || patch_env == 0;
    return f;
}

// 3x3 stride-1 layers take the halo kernel (conv_halo.hip) when the map is large enough for its 8x16 / 16x16 pixel
// tiles to fill the chip; variant choice from tools/conv_tune.py.
int halo_variant(const ConvGeom& g, const ConvForce& f) {
    if (!halo_conv_eligible(g)) return 0;
    if (f.halo >= 0) return f.halo;
    // measured in the training step (preset s, 32 images): the halo kernel wins on maps of 80x80 and more
    // (16x16-pixel tiles: 63 vs 81 us for 128->64 @80x80) and on 40x40 with exactly two 64-channel wave columns;
    // on smaller maps / other widths its tiles are too few or half empty and the gather kernel is level or better
    if ((long)g.Hg * g.Wg >= 80 * 80) return g.Cd >= 128 ? 2 : 3;
    if (g.Hg >= 40 && g.Wg >= 40 && g.Cd == 128) return 1;
    return 0;
}

// The row-block kernel (conv_rows.hip).  Returns 0 (not taken) or its variant (1 / 3 = 80 pixels x 64 channels per
// workgroup with four / three weight stages, 2 = 80 x 128, 4 = 160 x 64, 6 / 7 = 16-pixel-wide blocks, maps of any width).
// Default (tools/rows_bench.py, graph-replayed, 32 images, against the gather ring): 40-wide maps take the 160 x 64 tile
// (256->256: 83 -> 63 us, 64->64: 15.0 -> 12.8, 256->64: 38 -> 25), 20-wide maps too once the 80 x 64 tiling would put two
// workgroups on every CU (256->256: 35 -> 24 us), otherwise 80 x 64 (128->128: 17.8 -> 11.7, 512->64: 42.6 -> 21.5).
int rows_variant(const ConvGeom& g, const ConvForce& f) {
    const int el = rows_conv_eligible(g);
    if (!el || f.rows_off) return 0;
    // narrow layers (fewer than 64 destination channels): 20 x 16 pixels x 32 channels.  Ahead of the gather kernels with a full
    // 32-channel source chunk (64->32 @80x80 forward 28.4 -> 21.0 us, its 32->64 data gradient 26.1 -> 18.6; 32->16 @160x160
    // forward 41.9 -> 36.5), behind them with a 16-channel source (half-empty chunks): there only when forced
    if (el == 3) return (f.rows == 7 || (f.rows_wide16_auto && g.Cs % 32 == 0)) ? 7 : 0;
    if (f.rows == 6) return 6;                               // 16-pixel-wide blocks, any map width
    // wider maps: 10 x 16-pixel blocks x 64 channels beat the halo kernel where the layer has exactly one 64-channel tile
    // (64->64 @80x80 35 -> 31 us forward, 31.5 -> 26.8 data gradient; 128->64 forward 51.5 -> 41.5; 64->64 @160x160 104 -> 97)
    if (el == 2) return f.rows_wide16_auto && g.Cd == 64 && g.Cs >= 64 ? 6 : 0;
    if (f.rows >= 1 && f.rows <= 4) return f.rows == 2 && g.Cd <= 64 ? 1 : f.rows;
    if (g.Wg == 40) return 4;
    const long wgs = (long)g.N * ((g.Hg + 3) / 4) * ((g.Cd + 63) / 64);
    return wgs >= 512 ? 4 : 3;
}

// Where the ring kernel is used: `ring` = 1 (yolo_conv_tune_set) wherever it can run, 0 never, -1 (the default) where
// tools/ring_tune.py measured it ahead of the gather kernel on MI355X: maps of 40x40 and below with K >= 256 (every step
// a full cache line per row, half the barriers, the load of step t+1 under the MFMAs of step t), and 80x80 maps with
// K >= 1024.  Larger maps are HBM-bound streams that want the gather kernel's occupancy (12 KB of LDS per workgroup
// instead of 48+).  A parity class (ostep 2) counts with the pixels of the whole data gradient.
bool ring_wanted(const ConvGeom& g, int dtype, const void* src, const void* wm, const void* dst) {
    const int mode = conv_tune().ring;
    if (mode == 0) return false;
    if (mode < 0) {
        const int steps = g.ntaps * ((g.Cs + 63) / 64);
        const long all_pix = (long)g.N * g.Hd * g.Wd;
        if (!((all_pix <= 60000 && (steps >= 4 || g.ostep == 2)) || (all_pix <= 240000 && steps >= 16))) return false;
    }
    return ring_conv_eligible(g, dtype, src, wm, dst);
}

// Ring tile.  Pixel tiles of 128 while that still gives every CU a workgroup, else 64; channel tiles of 128 for wide
// layers while the grid stays at a workgroup per CU, else 64 (32 for <= 32 channels).  K-step and ring depth from
// tools/conv_tune.py (see the table in DESIGN.md).
RingTile ring_tile(const ConvGeom* gs, int n) {
    const int Cd = gs[0].Cd;
    long pix_tiles128 = 0, pix_tiles64 = 0;
    for (int c = 0; c < n; ++c) {
        const long pix = (long)gs[c].N * gs[c].Hg * gs[c].Wg;
        pix_tiles128 += (pix + 127) / 128;
        pix_tiles64 += (pix + 63) / 64;
    }
    RingTile t;
    auto wgs = [&](int bm, int bn) { return (bm == 128 ? pix_tiles128 : pix_tiles64) * ((Cd + bn - 1) / bn); };
    t.bn = Cd > 64 ? 128 : (Cd > 32 ? 64 : 32);
    t.bm = 128;
    if (t.bn == 128 && wgs(128, 128) < 256) t.bn = 64;
    if (t.bn != 32 && wgs(128, t.bn) < 256) t.bm = 64;
    const ConvTune& tu = conv_tune();
    if (tu.bn == 32 || tu.bn == 64 || tu.bn == 128) t.bn = tu.bn;
    if (tu.bm == 64 || tu.bm == 128) t.bm = tu.bm;
    t.bk = 64;
    if (tu.bk == 32 || tu.bk == 64) t.bk = tu.bk;
    if (t.bn == 32) { t.bm = 128; t.bk = 64; }                // the 32-channel tile exists for 64-deep steps only
    t.nst = 2;
    if (tu.nst >= 2 && tu.nst <= 4) t.nst = tu.nst;
    return t;
}

// Gather tile width (tools/conv_tune.py on MI355X): the widest channel tile that still yields one workgroup per CU --
// small maps with many channels (20x20, K in the thousands) otherwise run ~100 workgroups through a 144-step
// K loop on a 256-CU chip; narrower tiles than that only add LDS reads per MFMA.  One-tap convs whose source
// stays in the 256 MB Infinity Cache prefer 64-wide tiles (re-reading the source per channel tile is cheap there).
int conv_tile_bn(const ConvGeom& g) {
    const long tm = ((long)g.N * g.Hg * g.Wg + 127) / 128;   // pixel tiles (BM, conv_dev.h)
    auto blocks = [&](int bn) { return tm * ((g.Cd + bn - 1) / bn); };
    int bn = g.Cd > 64 ? 128 : (g.Cd > 32 ? 64 : 32);
    const long src_bytes = (long)g.N * g.Hs * g.Ws * g.lds * 2;
    if (bn == 128 && g.ntaps == 1 && src_bytes <= (128L << 20)) bn = 64;
    while (bn > 32 && blocks(bn) < 256) bn >>= 1;
    const ConvTune& tu = conv_tune();                        // overrides: tuning runs and variant-forcing tests only
    if (tu.bn == 32 || tu.bn == 64 || tu.bn == 128) bn = tu.bn;
    return bn;
}

}  // namespace

ConvChoice conv_select(const ConvGeom* gs, int n, int cls, int dtype, const void* src, const void* wm, const void* dst, int algo) {
    const ConvGeom& g = gs[cls];
    ConvChoice ch{};                                          // CONV_VALU
    // 1. the caller's algo; 2. no MFMA kernel for this problem: the VALU / fp32 kernels (algo 2: an error)
    if (algo == 1) return ch;
    if (!mfma_conv_eligible(g, dtype, src, wm, dst)) { ch.kind = algo == 2 ? CONV_NONE : CONV_VALU; return ch; }
    const ConvForce f = conv_force();
    if (n == 4) {                                             // stride-2 data gradient: one launch for the four parity classes?
        bool all_mfma = true, all_ring = true;
        for (int c = 0; c < 4; ++c) {
            all_mfma = all_mfma && mfma_conv_eligible(gs[c], dtype, src, wm, dst);
            all_ring = all_ring && ring_wanted(gs[c], dtype, src, wm, dst);
        }
        ch.joint = 1;
        // 3. the dy patch once for all four classes (conv_up2.hip).  Measured on every stride-2 layer of the step
        // (tools/up2_bench.py, 32 images, ring -> patch): 32->64 @320x320 157 -> 98 us, 128->128 @160 145 -> 107, 256->256 @80
        // 114 -> 88, 128->128 @80 50 -> 35, 256->256 @40 40 -> 35, 256->512 @40 65 -> 56; with 16-byte stores 91 / 99 / 86 / 32 /
        // 36 / 56 us.  8x16 dy pixels x 64 dx channels per workgroup, 16x16 x 32 for layers of 32 channels
        if (all_mfma && !f.up2_off && up2_conv_eligible(gs, dtype)) { ch.kind = CONV_UP2; ch.variant = g.Cd <= 32 ? 16 : 8; return ch; }
        // 4. the ring kernel with the four classes as sub-problems
        if (all_ring) { ch.kind = CONV_RING; ch.ring = ring_tile(gs, 4); return ch; }
        ch.joint = 0;                                         // each class on its own, by the questions below
    }
    if ((ch.variant = rows_variant(g, f))) { ch.kind = CONV_ROWS; return ch; }                          // 5.
    if ((ch.variant = halo_variant(g, f))) { ch.kind = CONV_HALO; return ch; }                          // 6.
    if (ring_wanted(g, dtype, src, wm, dst)) { ch.kind = CONV_RING; ch.ring = ring_tile(&g, 1); return ch; }   // 7.
    ch.kind = CONV_GATHER;                                                                              // 8.
    ch.bn = conv_tile_bn(g);
    return ch;
}

namespace {

// launches what conv_select chose for ONE geometry (wm = its packed weight matrix)
int launch_choice(const ConvChoice& ch, const ConvGeom& g, const void* src, const void* wm, const float* bias, void* dst,
                  int accumulate, int dtype, hipStream_t st) {
    if (ch.kind == CONV_NONE) return YOLO_ERR_ARG;            // MFMA demanded but the shape is not eligible
    if (ch.kind == CONV_VALU) return valu_conv_launch(g, src, wm, bias, dst, accumulate, dtype, st);
    if ((long)g.N * g.Hg * g.Wg == 0) return YOLO_OK;
    const long off0 = 0;
    switch (ch.kind) {
        case CONV_ROWS: return rows_conv_launch(g, ch.variant, src, wm, bias, dst, accumulate, dtype, st);
        case CONV_HALO: return halo_conv_launch(g, ch.variant, src, wm, bias, dst, accumulate, dtype, st);
        case CONV_RING: return ring_conv_launch(&g, 1, ch.ring, &off0, (long)g.Cd * g.Kpad, src, wm, bias, dst, accumulate, dtype, st);
        default: return mfma_conv_launch(g, ch.bn, src, wm, bias, dst, accumulate, dtype, st);
    }
}

ConvGeom fwd_geom(int ldx, int ldy, float* stats_acc, int N, int H, int W, int Cin, int OH, int OW, int Cout, int k, int stride) {
    ConvGeom g;
    g.stats = stats_acc;
    g.acc2 = nullptr; g.ld2 = 0;
    g.act = 0; g.res = nullptr; g.ldr = 0;
    g.N = N; g.Hs = H; g.Ws = W; g.Cs = Cin; g.lds = ldx;
    g.Hd = OH; g.Wd = OW; g.Cd = Cout; g.ldd = ldy; g.Hg = OH; g.Wg = OW;
    g.ostep = 1; g.ooff_h = 0; g.ooff_w = 0; g.sstride = stride;
    int kh[9], kw[9];
    g.ntaps = conv_taps(0, k, stride, 0, g.dh, g.dw, kh, kw);
    g.K = g.ntaps * Cin; g.Kpad = round_up32(g.K);
    return g;
}

// data gradient, parity class c (stride 2: four classes; stride 1: c = 0)
ConvGeom dgrad_geom(int lddy, int lddx, int N, int H, int W, int Cin, int OH, int OW, int Cout, int k, int stride, int c) {
    ConvGeom g;
    g.stats = nullptr;
    g.acc2 = nullptr; g.ld2 = 0;
    g.act = 0; g.res = nullptr; g.ldr = 0;
    g.N = N; g.Hs = OH; g.Ws = OW; g.Cs = Cout; g.lds = lddy;
    g.Hd = H; g.Wd = W; g.Cd = Cin; g.ldd = lddx;
    int kh[9], kw[9];
    g.ntaps = conv_taps(1, k, stride, c, g.dh, g.dw, kh, kw);
    g.K = g.ntaps * Cout; g.Kpad = round_up32(g.K);
    if (stride == 1) {
        g.Hg = H; g.Wg = W; g.ostep = 1; g.ooff_h = 0; g.ooff_w = 0; g.sstride = 1;
    } else {
        int ph = c >> 1, pw = c & 1;
        g.Hg = ph == 0 ? (H + 1) / 2 : H / 2;
        g.Wg = pw == 0 ? (W + 1) / 2 : W / 2;
        g.ostep = 2; g.ooff_h = ph; g.ooff_w = pw; g.sstride = 1;
    }
    return g;
}

// dx[N,H,W,Cin] (= or +=) conv^T(dy[N,OH,OW,Cout]); wb = dgrad-packed buffer from yolo_conv_pack_weights(mode 1)
int conv2d_dgrad_impl(const void* dy, int lddy, const void* wb, void* dx, int lddx, const void* acc2, int ld2, int N, int H,
                      int W, int Cin, int OH, int OW, int Cout, int k, int stride, int accumulate, int dtype, int algo,
                      hipStream_t st) {
    if (!conv_supported(k, stride, Cin, Cout)) return YOLO_ERR_ARG;
    size_t esz = dtype == YOLO_F32 ? 4 : 2;
    int ncls = stride == 2 ? 4 : 1;
    ConvGeom gs[4];
    long offs[4], off = 0;
    for (int c = 0; c < ncls; ++c) {
        gs[c] = dgrad_geom(lddy, lddx, N, H, W, Cin, OH, OW, Cout, k, stride, c);
        gs[c].acc2 = acc2; gs[c].ld2 = ld2;
        offs[c] = off;
        off += (long)Cin * gs[c].Kpad;
    }
    for (int c = 0; c < ncls; ++c) {
        const ConvGeom& g = gs[c];
        if (!(g.Hg > 0 && g.Wg > 0)) continue;                // an empty parity class (a map one pixel high or wide)
        const ConvChoice ch = conv_select(gs, ncls, c, dtype, dy, wb, dx, algo);
        if (ch.joint)                                         // one launch for the four parity classes
            return ch.kind == CONV_UP2 ? up2_conv_launch(gs, ch.variant, offs, off, dy, wb, dx, accumulate, dtype, st)
                                       : ring_conv_launch(gs, 4, ch.ring, offs, off, dy, wb, nullptr, dx, accumulate, dtype, st);
        int rc = launch_choice(ch, g, dy, (const char*)wb + offs[c] * esz, nullptr, dx, accumulate, dtype, st);
        if (rc) return rc;
    }
    return YOLO_OK;
}

}  // namespace

extern "C" {

// y[N,OH,OW,Cout] = conv(x[N,H,W,Cin], w) (+ bias); pad = k/2; wp = forward-packed weights in `dtype`.
// algo: 0 auto (MFMA when eligible), 1 generic VALU kernel, 2 MFMA or error.
// stats_acc (optional, needs bias == null): fp32 [8][2][Cout], pre-zeroed; receives sum(y) and sum(y^2) per channel
// (of the values as stored) for the BatchNorm that follows -- from the MFMA kernel's epilogue, no extra pass.
int yolo_conv2d_fwd(const void* x, int ldx, const void* wp, const float* bias, void* y, int ldy, float* stats_acc, int N,
                    int H, int W, int Cin, int OH, int OW, int Cout, int k, int stride, int dtype, int algo,
                    hipStream_t st) {
    if (!conv_supported(k, stride, Cin, Cout) || (stats_acc && bias)) return YOLO_ERR_ARG;
    int pad = k / 2;
    if (OH != (H + 2 * pad - k) / stride + 1 || OW != (W + 2 * pad - k) / stride + 1) return YOLO_ERR_ARG;
    ConvGeom g = fwd_geom(ldx, ldy, stats_acc, N, H, W, Cin, OH, OW, Cout, k, stride);
    return launch_choice(conv_select(&g, 1, 0, dtype, x, wp, y, algo), g, x, wp, bias, y, 0, dtype, st);
}

// Inference form of a fused Conv block (Model.fuse(): BatchNorm folded into the weights and a bias, reference
// src/model/model_blocks.py:36-37, src/utils/model_utils.py:72-118): y = act(conv(x) + bias) (+ res) in ONE launch -- bias,
// SiLU and the residual add of Residual / PSABlock ride in the epilogue of the MFMA kernels.  Returns 1 (nothing launched)
// when the shape / dtype has no MFMA kernel (fp32, unaligned channels): the caller then runs conv + the element-wise pass.
int yolo_conv2d_fwd_act(const void* x, int ldx, const void* wp, const float* bias, const void* res, int ldr, void* y, int ldy,
                        int N, int H, int W, int Cin, int OH, int OW, int Cout, int k, int stride, int act, int dtype,
                        hipStream_t st) {
    if (!conv_supported(k, stride, Cin, Cout) || (act != 0 && act != 1)) return YOLO_ERR_ARG;
    int pad = k / 2;
    if (OH != (H + 2 * pad - k) / stride + 1 || OW != (W + 2 * pad - k) / stride + 1) return YOLO_ERR_ARG;
    if (res != nullptr && ((ldr & 3) || (reinterpret_cast<uintptr_t>(res) & 7))) return 1;
    ConvGeom g = fwd_geom(ldx, ldy, nullptr, N, H, W, Cin, OH, OW, Cout, k, stride);
    g.act = act; g.res = res; g.ldr = ldr;
    const ConvChoice ch = conv_select(&g, 1, 0, dtype, x, wp, y, 0);
    if (ch.kind == CONV_VALU) return 1;
    return launch_choice(ch, g, x, wp, bias, y, 0, dtype, st);
}

int yolo_conv2d_dgrad(const void* dy, int lddy, const void* wb, void* dx, int lddx, int N, int H, int W, int Cin,
                      int OH, int OW, int Cout, int k, int stride, int accumulate, int dtype, int algo,
                      hipStream_t st) {
    return conv2d_dgrad_impl(dy, lddy, wb, dx, lddx, nullptr, 0, N, H, W, Cin, OH, OW, Cout, k, stride, accumulate, dtype, algo, st);
}

// dx = dgrad + dx + acc2: the data gradient accumulated into dx together with a SECOND tensor of dx's shape (row stride ld2)
// in the same epilogue -- a three-way gradient fan-in (C3K2: the chunk's half feeds the concat and a Residual whose own
// skip gradient is a third term) without an extra pass.  Stride 1 only.
int yolo_conv2d_dgrad_acc2(const void* dy, int lddy, const void* wb, void* dx, int lddx, const void* acc2, int ld2, int N, int H,
                           int W, int Cin, int OH, int OW, int Cout, int k, int stride, int dtype, int algo, hipStream_t st) {
    if (stride != 1 || acc2 == nullptr || (ld2 & 3) || (reinterpret_cast<uintptr_t>(acc2) & 7)) return YOLO_ERR_ARG;
    return conv2d_dgrad_impl(dy, lddy, wb, dx, lddx, acc2, ld2, N, H, W, Cin, OH, OW, Cout, k, stride, 1, dtype, algo, st);
}

// Which kernel a forward / data-gradient launch takes (tests assert that their shapes reach the variant they mean to cover):
// conv_select's answer for dense rows and aligned pointers, as kind * 1000 + width (include/yolo_hip.h)
int yolo_conv2d_plan(int N, int H, int W, int Cin, int OH, int OW, int Cout, int k, int stride, int mode, int cls, int dtype) {
    if (!conv_supported(k, stride, Cin, Cout)) return -1;
    ConvGeom gs[4];
    const int n = (mode == 1 && stride == 2) ? 4 : 1;
    if (n == 4 && (cls < 0 || cls > 3)) return -1;
    for (int c = 0; c < n; ++c)
        gs[c] = mode == 0 ? fwd_geom(Cin, Cout, nullptr, N, H, W, Cin, OH, OW, Cout, k, stride)
                          : dgrad_geom(Cout, Cin, N, H, W, Cin, OH, OW, Cout, k, stride, c);
    alignas(16) static const char nominal[16] = {};          // eligibility looks at alignment only
    const ConvChoice ch = conv_select(gs, n, n == 4 ? cls : 0, dtype, nominal, nominal, nominal, 0);
    switch (ch.kind) {
        case CONV_GATHER: return 1000 + ch.bn;
        case CONV_HALO: case CONV_ROWS: case CONV_UP2: return ch.kind * 1000 + ch.variant;
        case CONV_RING: return 3000 + (ch.ring.bm == 64 ? 500 : 0) + ch.ring.bn;
        default: return 0;
    }
}

}  // extern "C"
