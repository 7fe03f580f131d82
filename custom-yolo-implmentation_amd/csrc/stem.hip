// Stem (first layer: 3 -> C, 3x3 stride 2 pad 1, reference src/model/backbone.py:38).
// Cin = 3 cannot feed the MFMA gather (8-channel packets), and a VALU direct conv cost 8 ms per step.
// Instead the image is unfolded ONCE into a K = 27 (+5 zero) column matrix -- reading the NCHW input
// tensor directly, so the NCHW->NHWC conversion disappears too -- and forward / weight-gradient run
// as 1x1 convolutions on the MFMA kernels.  k = ci*9 + kh*3 + kw is exactly the OIHW flattening, so
// weights and weight gradients are plain [Cout][27] views padded to 32.
#include "common.h"
#include "bn_coef.h"
#include "conv_dev.h"

namespace {

template <typename TI, typename TO>
__global__ void k_stem_im2col(const TI* __restrict__ img, TO* __restrict__ col, int N, int H, int W, int OH, int OW) {
    long total = (long)N * OH * OW;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        int ow = (int)(p % OW);
        long t = p / OW;
        int oh = (int)(t % OH);
        long n = t / OH;
        float v[32];
#pragma unroll
        for (int k = 27; k < 32; ++k) v[k] = 0.f;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            const TI* plane = img + (n * 3 + ci) * (long)H * W;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                int ih = 2 * oh + kh - 1;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    int iw = 2 * ow + kw - 1;
                    bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
                    v[ci * 9 + kh * 3 + kw] = ok ? to_f<TI>(plane[(long)ih * W + iw]) : 0.f;
                }
            }
        }
        TO* o = col + p * 32;
        constexpr int V = vec_of<TO>::N;
#pragma unroll
        for (int k = 0; k < 32; k += V) {
            float w[V];
#pragma unroll
            for (int j = 0; j < V; ++j) w[j] = v[k + j];
            store_pack<TO, V>(o + k, w);
        }
    }
}

template <typename P, typename T>
__global__ void k_stem_pack_w(const P* __restrict__ w, int Cout, T* __restrict__ out) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Cout * 32) return;
    int o = e >> 5, k = e & 31;
    out[e] = from_f<T>(k < 27 ? to_f<P>(w[o * 27 + k]) : 0.f);
}

template <typename P>
__global__ void k_stem_unpack_dw(const float* __restrict__ dw32, int Cout, P* __restrict__ dw) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Cout * 27) return;
    int o = e / 27, k = e - o * 27;
    dw[e] = from_f<P>(dw32[o * 32 + k]);
}

// ---- fused forward: y = W * unfold(img) straight from the NCHW fp32 image (no column tensor in HBM) --------------------
// A workgroup owns 128 consecutive output pixels of TWO output rows: the 3 channels x 5 input rows it needs (257
// columns each) are staged once in LDS, one 16-byte load per lane = one row segment per wave instruction; every lane then gathers its MFMA B fragment
// (8 consecutive k of one pixel; k = ci*9 + kh*3 + kw, so row = k/3 and column offset = k%3) from LDS and the A
// fragments (weights [Cout][32], L2-resident) from global memory: one 16x16x32 MFMA per (16 channels x 16 pixels).
// Epilogue: 8-byte channel groups per lane, BatchNorm batch statistics of the rounded values (the pieces of conv_dev.h).
constexpr int STEM_SEG = 128;
constexpr int STEM_ROWW = 2 * STEM_SEG + 1;
constexpr int STEM_IR = 5;          // input rows per channel for TWO output rows (the middle one is shared)
constexpr int STEM_ROWS = 3 * STEM_IR;
constexpr int STEM_C0 = 3;          // staged column of image column 2*ow0 - 1: a 16-byte packet starts at [..][4]
typedef float StemRow[STEM_ROWW + 7];

// ---- the tile of the three kernels below, once ---------------------------------------------------------------------------
// Linear tile index -> (image, first of two output rows, first of 128 output pixels); the segment runs fastest.
struct StemTile {
    int n, oh0, ow0;
    __host__ __device__ constexpr int iw0() const { return 2 * ow0 - 1; }     // image column of staged column STEM_C0
};
__host__ __device__ constexpr int stem_segs(int OW) { return (OW + STEM_SEG - 1) / STEM_SEG; }
__host__ __device__ constexpr int stem_ohp(int OH) { return (OH + 1) >> 1; }
template <typename I>               // I: the index type the caller divides in (the forward's block index is 32-bit)
__host__ __device__ constexpr StemTile stem_tile(I tl, int segs, int ohp) {
    return StemTile{(int)(tl / segs / ohp), (int)(tl / segs % ohp) * 2, (int)(tl % segs) * STEM_SEG};
}
constexpr long stem_tiles(int N, int OH, int OW) { return (long)N * stem_ohp(OH) * stem_segs(OW); }
static_assert(stem_tile((2L * 10 + 7) * 3 + 2, 3, 10).n == 2 && stem_tile(83L, 3, 10).oh0 == 14 && stem_tile(83u, 3, 10).ow0 == 256 &&
              stem_tile(83, 3, 10).iw0() == 511 && stem_tiles(9, 232, 4) == 1044, "tile decode");

constexpr bool stem_shape_ok(int H, int W, int OH, int OW) { return OH == (H - 1) / 2 + 1 && OW == (W - 1) / 2 + 1; }

// The channel-tile counts CT = Cout / 16 the three kernels are instantiated for, once: STEM_DISPATCH_CT runs its statement with CT a
// constant (any other count: YOLO_ERR_ARG, as YOLO_DISPATCH_T does for a dtype), stem_ct_ok is yolo_stem_conv_eligible's table.
#define STEM_CTS(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(6, __VA_ARGS__) X(8, __VA_ARGS__)
#define STEM_CT_CASE(N, ...) case N: { constexpr int CT = N; __VA_ARGS__; } break;
#define STEM_DISPATCH_CT(ct, ...) switch (ct) { STEM_CTS(STEM_CT_CASE, __VA_ARGS__) default: return YOLO_ERR_ARG; }
#define STEM_CT_IS(N, ct) || (ct) == N
constexpr bool stem_ct_ok(int ct) { return false STEM_CTS(STEM_CT_IS, ct); }
static_assert(stem_ct_ok(1) && stem_ct_ok(6) && stem_ct_ok(8) && !stem_ct_ok(0) && !stem_ct_ok(5) && !stem_ct_ok(7) && !stem_ct_ok(9), "CT list");

// Unfold column k = ci*9 + kh*3 + kw -> row of the 3 x 5 staged window (for output row j of the pair add 2*j) and column offset
// (pixel p reads staged column STEM_C0 + 2*p + col); k >= 27 is the zero padding of K to 32 and reads nothing: row < 0.
struct StemTap { int row, col; };
__host__ __device__ constexpr StemTap stem_tap(int k) {
    const int ci = k / 9, r3 = k / 3;                    // kh = r3 - ci*3, kw = k - r3*3: two divisions, the forward decodes 8 taps per pixel
    return StemTap{k < 27 ? ci * STEM_IR + (r3 - ci * 3) : -1, k - r3 * 3};
}
constexpr bool stem_tap_is(int k, int ci, int kh, int kw) { return stem_tap(k).row == ci * STEM_IR + kh && stem_tap(k).col == kw; }
static_assert(stem_tap_is(0, 0, 0, 0) && stem_tap_is(5, 5 / 9, 5 / 3 % 3, 5 % 3) && stem_tap_is(13, 1, 1, 1) && stem_tap_is(17, 1, 2, 2) &&
              stem_tap_is(26, 26 / 9, 26 / 3 % 3, 26 % 3) && stem_tap_is(26, 2, 2, 2) && stem_tap(27).row < 0 && stem_tap(31).row < 0, "tap map");

// Image-row stager.  rows[ci*5 + ir][STEM_C0 + c] = image (n, ci), row 2*oh0 - 1 + ir, column iw0 + c for c in [0, 257).  Contract:
//  * every thread of the workgroup calls it; the barrier before it (the previous tile's readers are done) and the one after it
//    (the rows are published) are the caller's;
//  * a row above or below the image and a column at or past W hold 0 -- the conv's padding; the zero is SELECTED, never a product,
//    so a NaN / Inf outside the window does not enter (tests/test_gpu_nonfinite.py); the address of such an element is clamped to
//    row 0 / column 2*ow0, which exist, and there is no branch between the loads;
//  * the left-edge column iw0 is read from the image only when ow0 > 0 (for ow0 = 0 it is the padding column -1: zero, no read);
//  * W % 4 == 0: one 16-byte load per lane = one row segment per wave instruction (a lane's four columns exist together or not
//    at all), a wave's (up to four) row segments are ALL in flight before the first LDS store; any other W: the scalar path.
// The forward calls it.  k_stem_wgrad and k_stem_bn_wgrad carry the same text in their tile loops under the same contract (the second
// with its dz arithmetic between the halves): called from there it cost 0.4 % of either kernel.  Change all three together.
constexpr int STEM_RPW = (STEM_ROWS + 3) / 4;
struct StemRowRegs { float4 v[STEM_RPW]; float edge[STEM_RPW]; };

__device__ __forceinline__ void stem_rows_load(StemRowRegs& s, const float* __restrict__ img, const StemTile t, int H, int W,
                                               int lane, int wave) {
    const int c = lane * 4;
#pragma unroll
    for (int k = 0; k < STEM_RPW; ++k) {
        const int r = wave + 4 * k, rr = r < STEM_ROWS ? r : 0;
        const int ci = rr / STEM_IR, ir = rr - ci * STEM_IR;
        const int ih = 2 * t.oh0 + ir - 1;
        const bool rok = ih >= 0 && ih < H;
        const float* src = img + (((long)t.n * 3 + ci) * H + (rok ? ih : 0)) * (long)W + 2 * t.ow0;
        const bool cok = 2 * t.ow0 + c < W;                                             // W % 4 == 0: all four or none
        s.v[k] = *reinterpret_cast<const float4*>(src + (cok ? c : 0));
        if (!(rok && cok)) s.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        s.edge[k] = (lane == 0 && t.ow0 > 0) ? src[-1] : 0.f;
        if (!rok) s.edge[k] = 0.f;
    }
}

__device__ __forceinline__ void stem_rows_store(StemRow* rows, const StemRowRegs& s, int lane, int wave) {
    const int c = lane * 4;
#pragma unroll
    for (int k = 0; k < STEM_RPW; ++k) {
        const int r = wave + 4 * k;
        if (r < STEM_ROWS) {
            *reinterpret_cast<float4*>(&rows[r][STEM_C0 + 1 + c]) = s.v[k];
            if (lane == 0) rows[r][STEM_C0] = s.edge[k];
        }
    }
}

__device__ __forceinline__ void stem_rows_scalar(StemRow* rows, const float* __restrict__ img, const StemTile t, int H, int W, int tid) {
    for (int idx = tid; idx < STEM_ROWS * STEM_ROWW; idx += 256) {
        const int r = idx / STEM_ROWW, c = idx - r * STEM_ROWW;
        const int ci = r / STEM_IR, ir = r - ci * STEM_IR;
        const int ih = 2 * t.oh0 + ir - 1, iw = t.iw0() + c;
        const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
        rows[r][STEM_C0 + c] = ok ? img[(((long)t.n * 3 + ci) * H + ih) * (long)W + iw] : 0.f;
    }
}

__device__ __forceinline__ void stem_stage_rows(StemRow* rows, const float* __restrict__ img, const StemTile t, int H, int W, int tid,
                                                int lane, int wave) {
    if ((W & 3) == 0) {
        StemRowRegs s;
        stem_rows_load(s, img, t, H, W, lane, wave);
        stem_rows_store(rows, s, lane, wave);
    } else {
        stem_rows_scalar(rows, img, t, H, W, tid);
    }
}

template <typename T, int CT>
__global__ __launch_bounds__(256) void k_stem_conv(const float* __restrict__ img, const T* __restrict__ wp,
                                                   T* __restrict__ y, int ldy, float* __restrict__ stats, int N, int H,
                                                   int W, int OH, int OW, int Cout, const float* __restrict__ bias, int act) {
    typedef mfma_ops<T> ops;
    typedef typename ops::frag frag;
    __shared__ __attribute__((aligned(16))) StemRow rows[STEM_ROWS];
    __shared__ float sacc[2][16 * CT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, kg = lane >> 4;
    const StemTile t = stem_tile(blockIdx.x, stem_segs(OW), stem_ohp(OH));
    const int n = t.n, oh0 = t.oh0, ow0 = t.ow0;
    stem_stage_rows(rows, img, t, H, W, tid, lane, wave);
    stats_zero(&sacc[0][0], 2 * 16 * CT, tid, 256);         // before the barrier that publishes the rows: the statistics need no extra one
    frag a[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) a[ct] = *reinterpret_cast<const frag*>(wp + (long)(ct * 16 + fr) * 32 + kg * 8);
    __syncthreads();
    // a wave owns four 16-pixel tiles: tile id wave*4 + i = (output row j) * 8 + (tile within the 128-pixel segment)
    f32x4 acc[4][CT];                                    // [pixel tile][channel block]
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int tl = wave * 4 + i, j = tl >> 3;
        const int p = (tl & 7) * 16 + fr;                   // pixel of this lane's B column
        live[i] = ow0 + p < OW && oh0 + j < OH;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const StemTap tap = stem_tap(kg * 8 + e);
            v[e] = (tap.row >= 0 && live[i]) ? rows[tap.row >= 0 ? tap.row + 2 * j : 0][2 * p + tap.col + STEM_C0] : 0.f;
        }
        frag b;
#pragma unroll
        for (int e = 0; e < 8; ++e) b[e] = from_f<T>(v[e]);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            acc[i][ct] = ops::mma(a[ct], b, z);
        }
    }
    // lane holds channels ct*16 + kg*4 .. +3 of its tile's pixel fr
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!live[i]) continue;
        const int tl = wave * 4 + i;
        T* drow = y + (((long)n * OH + oh0 + (tl >> 3)) * OW + ow0 + (tl & 7) * 16 + fr) * (long)ldy;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[i][ct][r];
            if (bias != nullptr) {                              // fused inference (BatchNorm folded in): act(conv + b)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += bias[ct * 16 + kg * 4 + r];
            }
            if (act) fused_epilogue<T>(v, act, nullptr, 0);
            store_pack<T, 4>(drow + ct * 16 + kg * 4, v);
        }
    }
    if (stats != nullptr) {                                 // pixels past the row / image end hold 0
        stats_lane_sums<T, 4, CT>(acc, &sacc[0][0], 16 * CT, 0, kg * 4, fr);
        __syncthreads();
        stats_flush(&sacc[0][0], 16 * CT, stats, 0, Cout, tid, 256);
    }
}

// ---- weight gradient straight from the NCHW image: dW[co][k] = sum_p dY[p][co] * unfold(img)[p][k] -----------------
// Same tile as the forward (two output rows x 128 pixels, the 3 x 5 input row segments staged once in LDS) plus the
// tile's dY rows in their natural [pixel][channel] order.  The reduction index is the pixel: per group of 32 consecutive
// output pixels the dY^T fragments come out of LDS through the transposing read (as in k_wgrad2) and the unfold
// fragments are gathered from the staged image rows (8 consecutive pixels of one k = (ci, kh, kw) per lane, rounded
// to the compute dtype exactly as the column tensor was).  A workgroup walks tiles with a grid stride, keeps
// [Cout][32] sums per wave in registers, combines its waves in LDS and stores ONE partial matrix;
// k_stem_wgrad_reduce sums the workgroups straight into the OIHW gradient.  No column tensor exists any more.
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

template <typename T>
__device__ __forceinline__ typename mfma_ops<T>::frag stem_tr_frag(const T* p_lo, const T* p_hi) {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p_lo);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p_hi);
    s16x8 both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(typename mfma_ops<T>::frag, both);
}

constexpr int stem_ldy(int ct) { return ct == 4 ? 72 : ct == 8 ? 144 : ct * 16 + (ct == 2 ? 0 : 8); }

// Unfold fragments of a pixel run, for the two kernels whose reduction index is the pixel: fb[nt][e] = unfold column tap[nt] (the lane's
// k = nt*16 + i16) of output pixel px + e of output row j of the pair, e = 0..7, from the staged rows, rounded to T exactly as the column
// tensor was.  G3: g3[nt] += the rounded values of the run's first `nlive` pixels, the ones that exist (a pixel past the row / image
// end still has taps inside the image); without G3 nothing of it is compiled.
template <typename T, bool G3>
__device__ __forceinline__ void stem_gather_run(typename mfma_ops<T>::frag (&fb)[2], const StemRow* rows, const StemTap (&tap)[2], int j,
                                                int px, float* g3 = nullptr, bool rowok = false, int ow = 0, int OW = 0) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = tap[nt].row >= 0 ? rows[tap[nt].row < 0 ? 0 : tap[nt].row + 2 * j][2 * (px + e) + tap[nt].col + STEM_C0] : 0.f;
            const T xr = from_f<T>(x);
            fb[nt][e] = xr;
            if constexpr (G3) g3[nt] += (rowok && ow + e < OW) ? to_f<T>(xr) : 0.f;
        }
    }
}

// The four waves add their MFMA sums one after the other: wave 0 stores, waves 1, 2, 3 add, one barrier in front of each turn (fixed
// order: the result does not depend on the schedule).  a0 goes to the matrix [16*CT][32] at sum, and with NM = 2 a1 to the one behind it
// (NM = 1: a1 is not read): D rows = co (ct*16 + g*4 + r), cols = k (nt*16 + i16).  Two matrices share the turns, so a second one
// costs no barrier; also(first) runs inside the wave's turn too: the caller's other sums.  The barrier that publishes the last turn
// is the caller's.  The accumulators are two arrays, not acc[2][CT][2]: as one array k_stem_bn_wgrad took 4 more registers.
template <int NM, int CT, typename F>
__device__ __forceinline__ void stem_wave_combine(float* sum, const f32x4 (&a0)[CT][2], const f32x4 (&a1)[CT][2], int wave, int g, int i16,
                                                  F also) {
    for (int wv = 0; wv < 4; ++wv) {
        __syncthreads();
        if (wave == wv) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* e = &sum[(ct * 16 + g * 4 + r) * 32 + nt * 16 + i16];
                        e[0] = wv == 0 ? a0[ct][nt][r] : e[0] + a0[ct][nt][r];
                        if constexpr (NM == 2) e[CT * 512] = wv == 0 ? a1[ct][nt][r] : e[CT * 512] + a1[ct][nt][r];
                    }
            also(wv == 0);
        }
    }
}

template <typename T, int CT>
__global__ __launch_bounds__(256) void k_stem_wgrad(const float* __restrict__ img, const T* __restrict__ dy, int ldy,
                                                    float* __restrict__ part, int N, int H, int W, int OH, int OW, long tiles) {
    typedef mfma_ops<T> ops;
    typedef typename ops::frag frag;
    constexpr int LDY = stem_ldy(CT), COUT = 16 * CT;
    __shared__ __attribute__((aligned(16))) StemRow rows[STEM_ROWS];
    __shared__ __attribute__((aligned(16))) T ys[2 * STEM_SEG * LDY];
    __shared__ float sum[COUT * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, c4 = 4 * (i16 & 3);
    const int segs = stem_segs(OW), ohp = stem_ohp(OH);
    f32x4 acc[CT][2];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[ct][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const StemTap tap[2] = {stem_tap(i16), stem_tap(16 + i16)};       // this lane's two unfold columns: k = nt*16 + i16
    for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const StemTile t = stem_tile(tl, segs, ohp);
        const int n = t.n, oh0 = t.oh0, ow0 = t.ow0;
        __syncthreads();                                    // the previous tile's fragments have been read
        // the row stager's text (contract: at stem_rows_load), not a call: as a call this loop measured 0.4 % slower
        const int iw0 = t.iw0();
        if ((W & 3) == 0) {
            constexpr int RPW = STEM_RPW;
            float4 v[RPW];
            float edge[RPW];
            const int c = lane * 4;
#pragma unroll
            for (int k = 0; k < RPW; ++k) {
                const int r = wave + 4 * k, rr = r < 3 * STEM_IR ? r : 0;
                const int ci = rr / STEM_IR, ir = rr - ci * STEM_IR;
                const int ih = 2 * oh0 + ir - 1;
                const bool rok = ih >= 0 && ih < H;
                const float* src = img + (((long)n * 3 + ci) * H + (rok ? ih : 0)) * (long)W + 2 * ow0;
                const bool cok = 2 * ow0 + c < W;
                v[k] = *reinterpret_cast<const float4*>(src + (cok ? c : 0));
                if (!(rok && cok)) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                edge[k] = (lane == 0 && ow0 > 0) ? src[-1] : 0.f;
                if (!rok) edge[k] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < RPW; ++k) {
                const int r = wave + 4 * k;
                if (r < 3 * STEM_IR) {
                    *reinterpret_cast<float4*>(&rows[r][4 + c]) = v[k];
                    if (lane == 0) rows[r][3] = edge[k];
                }
            }
        } else {
            for (int idx = tid; idx < 3 * STEM_IR * STEM_ROWW; idx += 256) {
                const int r = idx / STEM_ROWW, c = idx - r * STEM_ROWW;
                const int ci = r / STEM_IR, ir = r - ci * STEM_IR;
                const int ih = 2 * oh0 + ir - 1, iw = iw0 + c;
                const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
                rows[r][3 + c] = ok ? img[(((long)n * 3 + ci) * H + ih) * (long)W + iw] : 0.f;
            }
        }
        // dY: 2 rows x 128 pixels x COUT channels, 16-byte chunks; pixels past the row / image end are zeros
        constexpr int CPP = COUT / 8;
        constexpr int DYR = 2 * STEM_SEG * CPP / 256;         // chunks per thread (CPP = COUT / 8: 2 ... 16), all in flight
        uint4 dv[DYR];
#pragma unroll
        for (int k = 0; k < DYR; ++k) {
            const int id = tid + 256 * k;
            const int px = id / CPP, ch = (id - px * CPP) * 8;
            const int j = px / STEM_SEG, p = px - j * STEM_SEG;
            const bool ok = oh0 + j < OH && ow0 + p < OW;
            dv[k] = *reinterpret_cast<const uint4*>(dy + (((long)n * OH + (ok ? oh0 + j : 0)) * OW + (ok ? ow0 + p : 0)) * (long)ldy + ch);
            if (!ok) dv[k] = make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < DYR; ++k) {
            const int id = tid + 256 * k;
            const int px = id / CPP, ch = (id - px * CPP) * 8;
            *reinterpret_cast<uint4*>(ys + px * LDY + ch) = dv[k];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {                       // wave w: the 32-pixel group w of both output rows
            const int px0 = wave * 32;
            frag fb[2];
            stem_gather_run<T, false>(fb, rows, tap, j, px0 + 8 * g);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const T* p = ys +(j * STEM_SEG + px0 + 8 * g + q) * LDY + ct * 16 + c4;
                const frag fa = stem_tr_frag<T>(p, p + 4 * LDY);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[ct][nt] = ops::mma(fa, fb[nt], acc[ct][nt]);
            }
        }
    }
    stem_wave_combine<1>(sum, acc, acc, wave, g, i16, [](bool) {});
    __syncthreads();
    float* o = part + (long)blockIdx.x * COUT * 32;
    for (int c = tid; c < COUT * 32; c += 256) o[c] = sum[c];
}

// dw[o][k] (OIHW (Cout,3,3,3) flat, k < 27) = sum over the workgroups' partial matrices; 32 lanes per element
template <typename P>
__global__ __launch_bounds__(256) void k_stem_wgrad_reduce(const float* __restrict__ part, int nslab, int Cout, P* __restrict__ dw) {
    const int e = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    if (e >= Cout * 27) return;
    const int o = e / 27, k = e - o * 27;
    float s = 0.f;
    for (int b = l; b < nslab; b += 32) s += part[((long)b * Cout + o) * 32 + k];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 32);
    if (l == 0) dw[e] = from_f<P>(s);
}

constexpr int STEM_WG_SLABS = 1024;

template <typename T>
int launch_stem_wgrad(const float* img, const void* dy, int ldy, float* part, int N, int H, int W, int OH, int OW, int Cout,
                      int* nslab, hipStream_t st) {
    const long tiles = stem_tiles(N, OH, OW);
    if (tiles <= 0) return YOLO_ERR_ARG;
    const int grid = (int)(tiles < STEM_WG_SLABS ? tiles : STEM_WG_SLABS);
    *nslab = grid;
    STEM_DISPATCH_CT(Cout / 16, hipLaunchKernelGGL((k_stem_wgrad<T, CT>), dim3(grid), dim3(256), 0, st, img, (const T*)dy, ldy, part, N, H,
                                                   W, OH, OW, tiles));
    return YOLO_LAUNCH_CHECK();
}

// ---- the stem's whole backward in ONE pass over (dout, y, image) --------------------------------------------------
// The stem takes no input gradient: the only consumer of BatchNorm's dy = A*dz + B*y + D (bn_bwd_coef) is the weight
// gradient, and there the channel co is an OUTPUT index, so the three per-channel constants factor out of the pixel sum:
//     dW[co][k] = A_co * G1[co][k] + B_co * G2[co][k] + D_co * G3[k]
//     G1 = sum_p dz[p][co] X[p][k],  G2 = sum_p y[p][co] X[p][k],  G3 = sum_p X[p][k] over the pixels that exist
// None of the sums needs A, B, D, which depend on (sum dz, sum dz*y) only: one kernel -- k_stem_wgrad's tile, staged image
// rows, grid-stride walk and one partial block per workgroup -- forms dz = dout * act'(y*scale + shift) in fp32, adds dz and
// dz*y into per-thread channel sums (unrounded, as channel_sums MODE 1 does), rounds dz once to T into one LDS tile, keeps y
// as stored in a second, and runs two MFMA accumulations per fragment on the same unfold fragments; G3 is a VALU sum of those
// fragments under the pixel's validity (a pixel past the row / image end still has taps inside the image).  dy is never
// formed, written or read.  The next tile's dout / y chunks are loaded while the current tile's fragments are multiplied.
// Partial block of a workgroup (fp32): G1[Cout][32], G2[Cout][32], G3[32], sum dz[Cout], sum dz*y[Cout].
constexpr int STEM_BN_SLABS = 512;                         // Cout = 32: 218 registers, two workgroups per CU on 256 CUs: one round
constexpr long stem_bn_block(int cout) { return (long)cout * 64 + 32 + 2 * cout; }

template <typename T, int CT, int ACT>
__global__ __launch_bounds__(256) void k_stem_bn_wgrad(const float* __restrict__ img, const T* __restrict__ dout, int ldd,
                                                       const T* __restrict__ y, int ldy, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, float* __restrict__ part, int N, int H,
                                                       int W, int OH, int OW, long tiles) {
    typedef mfma_ops<T> ops;
    typedef typename ops::frag frag;
    typedef pack_t<T, 8> chunk;
    constexpr int LDY = stem_ldy(CT), COUT = 16 * CT, TILE = 2 * STEM_SEG * LDY;
    // a thread keeps ONE 8-channel chunk (cpc) and walks pixels pl, pl + PPT, ...: its channel sums stay in registers
    constexpr int CPP = COUT / 8, PPT = 256 / CPP, NP = (2 * STEM_SEG + PPT - 1) / PPT;
    constexpr int RED = 17;                                  // row stride of the channel-sum exchange (16 values per thread)
    static_assert((2 * COUT * 32 + 32 + 256 * RED) * sizeof(float) <= 2 * TILE * sizeof(T), "the sums reuse the two tiles");
    __shared__ __attribute__((aligned(16))) StemRow rows[STEM_ROWS];
    __shared__ __attribute__((aligned(16))) T zs[2 * TILE];      // [0, TILE): dz rounded to T; [TILE, 2 TILE): y as stored
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, c4 = 4 * (i16 & 3);
    const int segs = stem_segs(OW), ohp = stem_ohp(OH);
    const int cpc = tid % CPP, pl = tid / CPP;
    const bool mine = pl < PPT;                              // Cout = 48, 96: four threads hold no chunk
    f32x4 acc1[CT][2], acc2[CT][2];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc1[ct][nt] = acc2[ct][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float g3[2] = {0.f, 0.f}, s[8], q[8], sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        s[j] = q[j] = 0.f;
        sc[j] = scale[cpc * 8 + j];
        sh[j] = shift[cpc * 8 + j];
    }
    const StemTap tap[2] = {stem_tap(i16), stem_tap(16 + i16)};       // this lane's two unfold columns: k = nt*16 + i16
    // dout and y of tile tl: 16-byte chunks, pixels past the row / image end are zeros (clamped addresses, no branch)
    chunk dv[NP], yv[NP];
    auto fetch = [&](long tl) {
        const StemTile t = stem_tile(tl, segs, ohp);
        const int n = t.n, oh0 = t.oh0, ow0 = t.ow0;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int px = pl + k * PPT, j = px / STEM_SEG, p = px - j * STEM_SEG;
            const bool ok = mine && px < 2 * STEM_SEG && oh0 + j < OH && ow0 + p < OW;
            const long pix = ((long)n * OH + (ok ? oh0 + j : 0)) * OW + (ok ? ow0 + p : 0);
            dv[k] = load_raw<T, 8>(dout + pix * ldd + cpc * 8);
            yv[k] = load_raw<T, 8>(y + pix * ldy + cpc * 8);
            if (!ok) dv[k] = yv[k] = chunk{};
        }
    };
    if (blockIdx.x < tiles) fetch(blockIdx.x);
    for (long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const StemTile t = stem_tile(tl, segs, ohp);
        const int oh0 = t.oh0, ow0 = t.ow0;
        __syncthreads();                                    // the previous tile's fragments have been read
        // the row stager's two halves as text, as in k_stem_wgrad: a wave's image row segments are in flight during the dz arithmetic
        const int n = t.n;
        constexpr int RPW = STEM_RPW;
        float4 v[RPW];
        float edge[RPW];
        const bool w4 = (W & 3) == 0;
        if (w4) {
            const int c = lane * 4;
#pragma unroll
            for (int k = 0; k < RPW; ++k) {
                const int r = wave + 4 * k, rr = r < 3 * STEM_IR ? r : 0;
                const int ci = rr / STEM_IR, ir = rr - ci * STEM_IR;
                const int ih = 2 * oh0 + ir - 1;
                const bool rok = ih >= 0 && ih < H;
                const float* src = img + (((long)n * 3 + ci) * H + (rok ? ih : 0)) * (long)W + 2 * ow0;
                const bool cok = 2 * ow0 + c < W;
                v[k] = *reinterpret_cast<const float4*>(src + (cok ? c : 0));
                if (!(rok && cok)) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                edge[k] = (lane == 0 && ow0 > 0) ? src[-1] : 0.f;
                if (!rok) edge[k] = 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int px = pl + k * PPT;
            if (mine && px < 2 * STEM_SEG) {
                float d[8], a[8];
                unpack<T, 8>(dv[k], d);
                unpack<T, 8>(yv[k], a);
                chunk z;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float dz = d[j] * act_grad(a[j] * sc[j] + sh[j], ACT);
                    s[j] += dz;
                    q[j] += dz * a[j];
                    z.v[j] = from_f<T>(dz);
                }
                *reinterpret_cast<chunk*>(zs + px * LDY + cpc * 8) = z;
                *reinterpret_cast<chunk*>(zs + TILE + px * LDY + cpc * 8) = yv[k];
            }
        }
        if (w4) {
            const int c = lane * 4;
#pragma unroll
            for (int k = 0; k < RPW; ++k) {
                const int r = wave + 4 * k;
                if (r < 3 * STEM_IR) {
                    *reinterpret_cast<float4*>(&rows[r][4 + c]) = v[k];
                    if (lane == 0) rows[r][3] = edge[k];
                }
            }
        }
        else stem_rows_scalar(rows, img, t, H, W, tid);
        if (tl + gridDim.x < tiles) fetch(tl + gridDim.x);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {                       // wave w: the 32-pixel group w of both output rows
            const int px0 = wave * 32;
            frag fb[2];
            stem_gather_run<T, true>(fb, rows, tap, j, px0 + 8 * g, g3, oh0 + j < OH, ow0 + px0 + 8 * g, OW);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const T* p = zs + (j * STEM_SEG + px0 + 8 * g + q4) * LDY + ct * 16 + c4;
                const frag fz = stem_tr_frag<T>(p, p + 4 * LDY);
                const frag fy = stem_tr_frag<T>(p + TILE, p + TILE + 4 * LDY);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    acc1[ct][nt] = ops::mma(fz, fb[nt], acc1[ct][nt]);
                    acc2[ct][nt] = ops::mma(fy, fb[nt], acc2[ct][nt]);
                }
            }
        }
    }
    // the two tiles become: G1 | G2 [COUT][32], G3 [32] (laid out as the partial block), the channel-sum exchange [256][RED]
    float* sum = reinterpret_cast<float*>(zs);
    float* g3s = sum + 2 * COUT * 32;
    float* red = g3s + 32;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {                         // the four 16-lane groups of a wave hold pixels 8g .. 8g+7 of a k
        g3[nt] += __shfl_xor(g3[nt], 16, 64);
        g3[nt] += __shfl_xor(g3[nt], 32, 64);
    }
    stem_wave_combine<2>(sum, acc1, acc2, wave, g, i16, [&](bool first) {       // G3 takes the same turns
        if (g == 0) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) g3s[nt * 16 + i16] = first ? g3[nt] : g3s[nt * 16 + i16] + g3[nt];
        }
    });
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[tid * RED + j] = s[j]; red[tid * RED + 8 + j] = q[j]; }
    __syncthreads();
    float* o = part + (long)blockIdx.x * stem_bn_block(COUT);
    for (int c = tid; c < 2 * COUT * 32 + 32; c += 256) o[c] = sum[c];
    // channel ch's two sums over the PPT threads that hold its chunk, in thread order
    for (int t = tid; t < 2 * COUT; t += 256) {
        const int which = t / COUT, ch = t - which * COUT, cl = ch >> 3, j = ch & 7;
        float a = 0.f;
        for (int rr = 0; rr < PPT; ++rr) a += red[(rr * CPP + cl) * RED + which * 8 + j];
        o[2 * COUT * 32 + 32 + t] = a;
    }
}

// One launch, one workgroup per output channel: lane k (32) x part (32) sums the workgroups' partial blocks in a fixed order
// in double, derives dbeta, dgamma, A, B, D (bn_bwd_coef_d) and forms dW = A*G1 + B*G2 + D*G3 in double -- B*G2 + D*G3
// cancel when |mean| / std is large, so the products are never rounded to fp32 before the sum.
template <typename P>
__global__ __launch_bounds__(1024) void k_stem_bn_wgrad_finalize(const float* __restrict__ part, int nslab, int Cout, float count,
                                                                 const void* __restrict__ gamma_, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, void* __restrict__ dgamma_,
                                                                 void* __restrict__ dbeta_, P* __restrict__ dw, int pdt) {
    __shared__ double red[5][32][33];
    const PIn gamma{gamma_, pdt}; const PIo dgamma{dgamma_, pdt}, dbeta{dbeta_, pdt};
    const int co = blockIdx.x, k = threadIdx.x & 31, sub = threadIdx.x >> 5;
    const long bs = stem_bn_block(Cout);
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int b = sub; b < nslab; b += 32) {
        const float* p = part + b * bs;
        a[0] += p[co * 32 + k];
        a[1] += p[(Cout + co) * 32 + k];
        a[2] += p[Cout * 64 + k];
        a[3] += p[Cout * 64 + 32 + co];
        a[4] += p[Cout * 64 + 32 + Cout + co];
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) red[i][sub][k] = a[i];
    __syncthreads();
    if (sub != 0) return;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double t = 0.0;
        for (int j = 0; j < 32; ++j) t += red[i][j][k];
        a[i] = t;
    }
    const BnBwdCoefD c = bn_bwd_coef_d(a[3], a[4], count, gamma, mean, invstd, co);
    if (k == 0) { dbeta.st(co, (float)c.dbeta); dgamma.st(co, (float)c.dgamma); }
    if (k < 27) dw[co * 27 + k] = from_f<P>((float)(c.A * a[0] + c.B * a[1] + c.D * a[2]));
}

template <typename T, int ACT>
int launch_stem_bn_wgrad(const float* img, const void* dout, int ldd, const void* y, int ldy, const float* scale,
                         const float* shift, float* part, int N, int H, int W, int OH, int OW, int Cout, int* nslab, hipStream_t st) {
    const long tiles = stem_tiles(N, OH, OW);
    if (tiles <= 0) return YOLO_ERR_ARG;
    const int grid = (int)(tiles < STEM_BN_SLABS ? tiles : STEM_BN_SLABS);
    *nslab = grid;
    STEM_DISPATCH_CT(Cout / 16, hipLaunchKernelGGL((k_stem_bn_wgrad<T, CT, ACT>), dim3(grid), dim3(256), 0, st, img, (const T*)dout, ldd,
                                                   (const T*)y, ldy, scale, shift, part, N, H, W, OH, OW, tiles));
    return YOLO_LAUNCH_CHECK();
}

template <typename T>
int launch_stem_conv(const float* img, const void* wp, void* y, int ldy, float* stats, int N, int H, int W, int OH, int OW,
                     int Cout, const float* bias, int act, hipStream_t st) {
    const long blocks = stem_tiles(N, OH, OW);
    if (blocks <= 0 || blocks > 0x7fffffffL) return YOLO_ERR_ARG;
    STEM_DISPATCH_CT(Cout / 16, hipLaunchKernelGGL((k_stem_conv<T, CT>), dim3((unsigned)blocks), dim3(256), 0, st, img, (const T*)wp, (T*)y,
                                                   ldy, stats, N, H, W, OH, OW, Cout, bias, act));
    return YOLO_LAUNCH_CHECK();
}

}  // namespace

extern "C" {

// img: (N,3,H,W) contiguous NCHW of img_dtype; col: [N*OH*OW][32] of col_dtype (an NHWC tensor with C = 32)
int yolo_stem_im2col(const void* img, int img_dtype, void* col, int col_dtype, int N, int H, int W, int OH, int OW,
                     hipStream_t st) {
    if (!stem_shape_ok(H, W, OH, OW)) return YOLO_ERR_ARG;
    long total = (long)N * OH * OW;
    int grid = (int)((total + 255) / 256 > 256 * 16 ? 256 * 16 : (total + 255) / 256);
    if (grid < 1) grid = 1;
#define STEM_LAUNCH(TI) YOLO_DISPATCH_T(col_dtype, hipLaunchKernelGGL((k_stem_im2col<TI, T>), dim3(grid), dim3(256), 0, st, (const TI*)img, (T*)col, N, H, W, OH, OW))
    switch (img_dtype) {
        case YOLO_F32:  STEM_LAUNCH(float); break;
        case YOLO_BF16: STEM_LAUNCH(bf16_t); break;
        case YOLO_F16:  STEM_LAUNCH(f16_t); break;
        default: return YOLO_ERR_DTYPE;
    }
#undef STEM_LAUNCH
    return YOLO_LAUNCH_CHECK();
}

// w: OIHW (Cout,3,3,3) -> out [Cout][32] (the forward-packed matrix of a 1x1 conv with Cin = 32)
int yolo_stem_pack_weights(const void* w, int w_dtype, int Cout, void* out, int out_dtype, hipStream_t st) {
    int grid = (Cout * 32 + 255) / 256;
#define PACK_LAUNCH(P) YOLO_DISPATCH_T(out_dtype, hipLaunchKernelGGL((k_stem_pack_w<P, T>), dim3(grid), dim3(256), 0, st, (const P*)w, Cout, (T*)out))
    switch (w_dtype) {
        case YOLO_F32:  PACK_LAUNCH(float); break;
        case YOLO_BF16: PACK_LAUNCH(bf16_t); break;
        case YOLO_F16:  PACK_LAUNCH(f16_t); break;
        default: return YOLO_ERR_DTYPE;
    }
#undef PACK_LAUNCH
    return YOLO_LAUNCH_CHECK();
}

// dw32: fp32 (Cout,32,1,1) gradient of the padded 1x1 weights -> dw OIHW (Cout,3,3,3) of dw_dtype
int yolo_stem_unpack_wgrad(const float* dw32, int Cout, void* dw, int dw_dtype, hipStream_t st) {
    int grid = (Cout * 27 + 255) / 256;
    YOLO_DISPATCH_T(dw_dtype, hipLaunchKernelGGL((k_stem_unpack_dw<T>), dim3(grid), dim3(256), 0, st, dw32, Cout, (T*)dw));
    return YOLO_LAUNCH_CHECK();
}

// 1 if yolo_stem_conv_fwd handles these arguments (fp32 NCHW image, bf16/f16 compute, Cout in {16,32,48,64,96,128})
int yolo_stem_conv_eligible(int img_dtype, int dtype, int Cout) {
    return img_dtype == YOLO_F32 && (dtype == YOLO_BF16 || dtype == YOLO_F16) && Cout % 16 == 0 && stem_ct_ok(Cout / 16);
}

// y[N][OH][OW][ld >= Cout] (dtype) = conv3x3 stride 2 pad 1 of img (N,3,H,W) fp32 NCHW with wp = yolo_stem_pack_weights
// output ([Cout][32], dtype); stats: optional [8][2][Cout] BatchNorm accumulator (sum, sum of squares of the stored values).
// bias (optional fp32 [Cout]) and act (0 identity, 1 SiLU): the fused-inference form act(conv + bias) of Model.fuse();
// not combined with stats (the statistics are those of the raw conv output).
int yolo_stem_conv_fwd(const float* img, const void* wp, void* y, int ldy, float* stats, int N, int H, int W, int OH, int OW,
                       int Cout, const float* bias, int act, int dtype, hipStream_t st) {
    if ((bias != nullptr || act) && stats != nullptr) return YOLO_ERR_ARG;
    if (act != 0 && act != 1) return YOLO_ERR_ARG;
    if (!yolo_stem_conv_eligible(YOLO_F32, dtype, Cout) || ldy < Cout) return YOLO_ERR_ARG;
    if (!stem_shape_ok(H, W, OH, OW)) return YOLO_ERR_ARG;
    if (dtype == YOLO_BF16) return launch_stem_conv<bf16_t>(img, wp, y, ldy, stats, N, H, W, OH, OW, Cout, bias, act, st);
    return launch_stem_conv<f16_t>(img, wp, y, ldy, stats, N, H, W, OH, OW, Cout, bias, act, st);
}

// number of partial matrices yolo_stem_wgrad may write: partial = fp32 [yolo_stem_wgrad_slabs()][Cout][32] scratch
int yolo_stem_wgrad_slabs(void) { return STEM_WG_SLABS; }

// dw OIHW (Cout,3,3,3) of dw_dtype = weight gradient of the stem conv from the fp32 NCHW image and dy[N][OH][OW][ldy >= Cout]
// (dtype bf16/f16; same eligibility as yolo_stem_conv_fwd).  Replaces unfold + 1x1 weight gradient + unpack.
int yolo_stem_wgrad(const float* img, const void* dy, int ldy, float* partial, void* dw, int dw_dtype, int N, int H, int W,
                    int OH, int OW, int Cout, int dtype, hipStream_t st) {
    if (!yolo_stem_conv_eligible(YOLO_F32, dtype, Cout) || ldy < Cout || (ldy & 7) || (reinterpret_cast<uintptr_t>(dy) & 15)) return YOLO_ERR_ARG;
    if (!stem_shape_ok(H, W, OH, OW)) return YOLO_ERR_ARG;
    int nslab = 0;
    const int rc = dtype == YOLO_BF16 ? launch_stem_wgrad<bf16_t>(img, dy, ldy, partial, N, H, W, OH, OW, Cout, &nslab, st)
                                      : launch_stem_wgrad<f16_t>(img, dy, ldy, partial, N, H, W, OH, OW, Cout, &nslab, st);
    if (rc) return rc;
    const int grid = (Cout * 27 + 7) / 8;
    YOLO_DISPATCH_T(dw_dtype, hipLaunchKernelGGL((k_stem_wgrad_reduce<T>), dim3(grid), dim3(256), 0, st, partial, nslab, Cout, (T*)dw));
    return YOLO_LAUNCH_CHECK();
}

// fp32 elements of the scratch yolo_stem_bn_wgrad needs: one partial block per workgroup
long yolo_stem_bn_wgrad_ws_elems(int Cout) { return STEM_BN_SLABS * stem_bn_block(Cout); }

// The stem's BatchNorm + activation backward AND its weight gradient in one pass (training mode; same eligibility as
// yolo_stem_conv_fwd): from the fp32 NCHW image, dout and the stored conv output y (both [N][OH][OW][ld >= Cout], dtype)
// and the forward's scale / shift / mean / invstd -> dw OIHW (Cout,3,3,3) of dw_dtype, dgamma / dbeta [Cout] of pdt.
// BatchNorm's input gradient is not formed.  No atomics: two launches of the same inputs give the same bits.
int yolo_stem_bn_wgrad(const float* img, const void* dout, int ldd, const void* y, int ldy, const float* scale, const float* shift,
                       const void* gamma, const float* mean, const float* invstd, float* partial, void* dw, int dw_dtype,
                       void* dgamma, void* dbeta, int N, int H, int W, int OH, int OW, int Cout, int act, int dtype, int pdt,
                       hipStream_t st) {
    if (!yolo_stem_conv_eligible(YOLO_F32, dtype, Cout) || !pdt_ok(pdt) || (act != 0 && act != 1)) return YOLO_ERR_ARG;
    if (ldd < Cout || (ldd & 7) || (reinterpret_cast<uintptr_t>(dout) & 15)) return YOLO_ERR_ARG;
    if (ldy < Cout || (ldy & 7) || (reinterpret_cast<uintptr_t>(y) & 15)) return YOLO_ERR_ARG;
    if (!stem_shape_ok(H, W, OH, OW)) return YOLO_ERR_ARG;
    int nslab = 0, rc;
#define STEM_BW_ACT(T) (act ? launch_stem_bn_wgrad<T, 1>(img, dout, ldd, y, ldy, scale, shift, partial, N, H, W, OH, OW, Cout, &nslab, st) \
                            : launch_stem_bn_wgrad<T, 0>(img, dout, ldd, y, ldy, scale, shift, partial, N, H, W, OH, OW, Cout, &nslab, st))
    rc = dtype == YOLO_BF16 ? STEM_BW_ACT(bf16_t) : STEM_BW_ACT(f16_t);
#undef STEM_BW_ACT
    if (rc) return rc;
    const float count = (float)((long)N * OH * OW);
    YOLO_DISPATCH_T(dw_dtype, hipLaunchKernelGGL((k_stem_bn_wgrad_finalize<T>), dim3(Cout), dim3(1024), 0, st, partial, nslab, Cout, count, gamma,
                                                 mean, invstd, dgamma, dbeta, (T*)dw, pdt));
    return YOLO_LAUNCH_CHECK();
}

}  // extern "C"
