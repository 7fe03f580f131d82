// Host-side interface between the conv translation units: every host function one of them calls in another is declared
// here and nowhere else.  Each kernel family answers "can I run this geometry at all?" (*_eligible) and launches; WHICH
// family and variant a problem takes is decided in one place, conv_select (conv_select.hip).
#pragma once
#include "common.h"
#include "conv_geom.h"

// ---- the choice
enum ConvKind {                 // the values are the thousands of yolo_conv2d_plan's code
    CONV_NONE = -1,             // algo 2 demanded an MFMA kernel and the problem has none
    CONV_VALU = 0,              // k_conv_generic / the LDS-tiled fp32 kernel (conv_generic.hip, conv_f32.hip)
    CONV_GATHER = 1,            // k_conv_mfma (conv_mfma.hip)
    CONV_HALO = 2,              // k_conv_halo (conv_halo.hip)
    CONV_RING = 3,              // k_conv_ring (conv_ring.hip)
    CONV_ROWS = 4,              // k_conv_rows (conv_rows.hip)
    CONV_UP2 = 5                // k_dgrad2_patch (conv_up2.hip)
};
struct RingTile { int bm, bn, nst, bk; };      // ring kernel: pixel tile, channel tile, ring depth, K-step
struct ConvChoice {
    int kind;                   // ConvKind
    int joint;                  // 1: ONE launch covers all four parity classes of a stride-2 data gradient (up2, ring)
    int variant;                // halo 1..4, rows 1..4 / 6 / 7, up2 8 / 16 (see the families' *_launch)
    int bn;                     // gather: channel tile 32 / 64 / 128
    RingTile ring;
};
// gs[0..n): one geometry (n = 1) or the four parity classes of a stride-2 data gradient (n = 4); the answer is for gs[cls].
// The three pointers are looked at for alignment only.  algo: 0 automatic, 1 VALU, 2 MFMA or CONV_NONE.
ConvChoice conv_select(const ConvGeom* gs, int n, int cls, int dtype, const void* src, const void* wm, const void* dst, int algo);

// ---- tune state (conv_select.hip; ConvTune: conv_geom.h)
ConvTune& conv_tune();
int conv_wide_flag();            // conv_mfma.hip: 16-byte epilogue stores: 2 (default) exchange by v_permlane16_swap, 1 by ds_bpermute, 0 off (YOLO_CONV_WIDE, yolo_conv_wide_set)

// ---- the addressing contract of the buffer descriptors: 32-bit byte counts and offsets over 2-byte elements, int pixel indices.
// elems = all that ONE descriptor covers (a tensor plus the row + pixel its base is shifted back by; a whole weight buffer)
static inline bool desc_addressable(long elems) { return elems < (1L << 30); }
static inline bool pixels_addressable(long npix) { return npix < (1L << 31); }

// ---- what the MFMA families share (conv_select.hip): 16-bit dtype, 8-channel source rows, 32-bit byte offsets / buffer
// descriptors in the gather, 32-bit pixel indices, 16-byte aligned operands, taps within one pixel of the centre
int mfma_conv_addressable(const ConvGeom& g, int dtype, const void* src, const void* wm, const void* dst);

// ---- the families.  Launches of gs[0..n) share source, destination tensor, channel counts and strides (n = 1, or the four
// parity classes; empty classes are skipped); wm_off[c] = element offset of class c's packed weight matrix inside wm,
// wm_elems = size of the whole buffer
int valu_conv_launch(const ConvGeom& g, const void* src, const void* wm, const float* bias, void* dst, int accumulate, int dtype,
                     hipStream_t st);                                                          // conv_generic.hip
int mfma_conv_eligible(const ConvGeom& g, int dtype, const void* src, const void* wm, const void* dst);   // conv_mfma.hip
int mfma_conv_launch(const ConvGeom& g, int bn, const void* src, const void* wm, const float* bias, void* dst, int accumulate,
                     int dtype, hipStream_t st);
int halo_conv_eligible(const ConvGeom& g);                                                     // conv_halo.hip
int halo_conv_launch(const ConvGeom& g, int variant, const void* src, const void* wm, const float* bias, void* dst,
                     int accumulate, int dtype, hipStream_t st);
int ring_conv_eligible(const ConvGeom& g, int dtype, const void* src, const void* wm, const void* dst);   // conv_ring.hip
int ring_conv_launch(const ConvGeom* gs, int n, const RingTile& t, const long* wm_off, long wm_elems, const void* src,
                     const void* wm, const float* bias, void* dst, int accumulate, int dtype, hipStream_t st);
int rows_conv_eligible(const ConvGeom& g);                                                     // conv_rows.hip
int rows_conv_launch(const ConvGeom& g, int variant, const void* src, const void* wm, const float* bias, void* dst, int accumulate,
                     int dtype, hipStream_t st);
int up2_conv_eligible(const ConvGeom* gs, int dtype);                                          // conv_up2.hip
int up2_conv_launch(const ConvGeom* gs, int variant, const long* wm_off, long wm_elems, const void* src, const void* wm, void* dst,
                    int accumulate, int dtype, hipStream_t st);
int f32_conv_eligible(const ConvGeom& g, const void* src, const void* wm, const void* dst);    // conv_f32.hip
int f32_conv_launch(const ConvGeom& g, const float* src, const float* wm, const float* bias, float* dst, int accumulate,
                    hipStream_t st);

// ---- weight gradient (conv_f32.hip, conv_mfma.hip, wgrad_mfma.hip)
int f32_wgrad_eligible(const void* x, int ldx, const void* dy, int ldy, int Cin, int Cout);
int f32_wgrad_launch(const float* x, int ldx, const float* dy, int ldy, float* dwp, int Kpad, int N, int H, int W, int Cin,
                     int OH, int OW, int Cout, int k, int stride, hipStream_t st);
int mfma_wgrad_eligible(int Cin, int Cout, int ldx, int ldy, int dtype, const void* x, const void* dy);
int mfma_wgrad_launch(const void* x, int ldx, const void* dy, int ldy, float* dwp, int Kpad, int N, int H, int W,
                      int Cin, int OH, int OW, int Cout, int k, int stride, int dtype, hipStream_t st);
long mfma_wgrad2_plan(int Kpad, int N, int H, int W, int Cin, int OH, int OW, int Cout, int k);
long mfma_wgrad2_ws_elems(int Kpad, int N, int H, int W, int Cin, int OH, int OW, int Cout, int k);
int mfma_wgrad2_launch(const void* x, int ldx, const void* dy, int ldy, float* part, void* dw_oihw, int dw_dtype, int Kpad,
                       int N, int H, int W, int Cin, int OH, int OW, int Cout, int k, int stride, int dtype, hipStream_t st);

// ---- depthwise kernels for 16-bit tensors with 8-channel alignment (dwconv.hip; -1 = does not qualify): the rows or the
// strip kernels, per shape (dw_takes_rows) unless dw_tune_set / YOLO_DW_KERNEL=strip|rows forces one
struct DwPlan {                 // rows kernels, one (N, H, W, C) map
    int cvb, ncy;               // channel groups (of 8) per workgroup, channel blocks (grid y)
    int ncol, ncb;              // columns per workgroup, column blocks per row
    int wg;                     // threads per workgroup
    int hb, nb, grid;           // forward / data gradient: band height, bands per image, grid x
    int hb_wg, nb_wg, grid_wg;  // weight gradient: the same (grid x = partial blocks written, before the cap by nslab)
};
DwPlan dw_plan(int N, int H, int W, int C);
int dw_tune_set(int variant);    // 0 per shape (default), 1 strip, 2 rows
bool dw_takes_rows(int N, int H, int W, int C, bool wgrad);
int dw16_launch(bool flip, const void* x, int ldx, const float* w, void* y, int ldy, int N, int H, int W, int C, int dtype,
                int accumulate, float* stats, hipStream_t st, const float* bias = nullptr, int act = 0);
// *nrows = partial blocks written (<= nslab): what k_dw_wgrad_finalize has to sum
int dw16_wgrad_launch(const void* x, int ldx, const void* dy, int ldy, float* partial, int nslab, int* nrows, int N, int H, int W,
                      int C, int dtype, hipStream_t st);

// ---- entry points of elementwise.hip that the VALU fallback chains
extern "C" int yolo_bn_stats_acc(const void* y, int ldy, long npix, int C, int dtype, float* acc, hipStream_t st);
extern "C" int yolo_copy_channels(const void* src, int ld_src, void* dst, int ld_dst, long npix, int C, int accumulate, int dtype,
                                  hipStream_t st);

static inline bool conv_supported(int k, int stride) { return (k == 1 && stride == 1) || (k == 3 && (stride == 1 || stride == 2)); }
// K = k * k * channels and its padding to 32 are `int` (ConvGeom, the packed weight rows): a problem whose packed row would
// not fit one is refused like an unsupported kernel size, before any such product is formed
static inline bool conv_supported(int k, int stride, int Cin, int Cout) {
    return conv_supported(k, stride) && Cin >= 0 && Cout >= 0 && (long)k * k * (Cin > Cout ? Cin : Cout) <= 2147483647L - 31;
}
