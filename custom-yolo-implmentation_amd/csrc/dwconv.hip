// Depthwise 3x3 (stride 1, pad 1) for 16-bit NHWC tensors: forward, data gradient (flipped taps) and weight gradient.
//
// The first form (k_dw3x3 in conv_generic.hip, kept for fp32 and unaligned tensors) fetched nine 16-byte neighbours
// per output through divergent border branches: 60-100 us on the 80x80x128 maps of the head against 21 us of HBM time.
// Here a thread owns 8 channels (one 16-byte packet) of a vertical strip of R output pixels: (R+2) x 3 packets are
// fetched up front through a buffer descriptor -- border packets are offsets beyond the descriptor's range, which the
// hardware returns as zeros, so there is no branch between the loads and all of them are in flight together -- and
// feed R x 9 x 8 FMAs: 4.5 loads per output for R = 4 instead of 9, horizontal reuse through the vector L1 (lanes of
// a wave that differ in the column fetch overlapping 1-KB runs).  The 9 x C fp32 taps of the workgroup's channels
// sit in LDS ([tap][half][channel group][4]: conflict-free 16-byte reads).
//
// The default form (k_dw3x3_rows, k_dw3x3_wgrad_rows) keeps the packet column and the buffer loads and walks a BAND of
// consecutive rows from top to bottom with a rolling window of input rows in registers: per output row only the three
// packets of the next input row are fetched (3 loads per output, the two halo rows of a band the only rows fetched
// twice), DW_PF rows ahead of the row being computed, and a workgroup stages its taps once for all its bands.  The plan
// (dw_plan) picks the columns per workgroup for the fewest idle columns and the band height for the grid; the strip
// kernels stay, as the form of the small maps (dw_takes_rows) and as a variant (yolo_dw_tune_set, YOLO_DW_KERNEL=strip / rows)
// that the rows kernels must match bit for bit.
#include <cstdlib>
#include <cstring>
#include "conv_host.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));

template <typename T> __device__ __forceinline__ void unpack8(const u32x4& v, float (&o)[8]);
template <> __device__ __forceinline__ void unpack8<bf16_t>(const u32x4& v, float (&o)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[2 * i] = __uint_as_float(v[i] << 16);
        o[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
}
template <> __device__ __forceinline__ void unpack8<f16_t>(const u32x4& v, float (&o)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // (a bit_cast of the vector ELEMENT to a half2 was miscompiled for i >= 1: channels 2..7 of every packet came out
        // wrong in fp16 while bf16 was exact -- found by the FSDP2 fp16 parity test, tests/test_gpu_kernels.py::test_depthwise)
        const unsigned int u = v[i];
        o[2 * i] = (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu));
        o[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16));
    }
}

struct DwGeom {
    int N, H, W, C, ldx, ldy;
    int cvb;        // channel groups (of 8) per workgroup
    int ncol;       // columns per workgroup
    int hb;         // rows per strip (strip kernels: R) / per band (rows kernels)
    int nsh;        // row strips / bands per image
    int ncb;        // column blocks per row
    long total;     // strips * column blocks * images
    const float* bias;   // fused inference (forward only): y = act(conv + bias); nullptr / 0 otherwise
    int act;
};

// taps of the workgroup's channels -> LDS, [tap][half][cvb][4]
template <bool FLIP>
__device__ __forceinline__ void stage_taps(float* wl, const float* __restrict__ w, int c0, int C, int cvb) {
    for (int i = threadIdx.x; i < cvb * 8 * 9; i += blockDim.x) {
        const int ch = i / 9, t = i - ch * 9;
        const float v = (c0 + ch < C) ? w[(long)(c0 + ch) * 9 + (FLIP ? 8 - t : t)] : 0.f;
        wl[((t * 2 + ((ch >> 2) & 1)) * cvb + (ch >> 3)) * 4 + (ch & 3)] = v;
    }
}

// the rows kernel's layout, [channel group][DW_TAP_LD]: a thread's 72 taps at constant offsets from ONE address ([tap][8]);
// 76 floats = 19 16-byte slots per group, odd, so the lanes of a 16-byte read fall on different slots
constexpr int DW_TAP_LD = 76;
constexpr size_t DW_TAP_MAX = 256 * DW_TAP_LD * sizeof(float);   // 76 KiB at 256 channel groups: above the default limit of dynamic LDS
template <bool FLIP>
__device__ __forceinline__ void stage_taps_rows(float* wl, const float* __restrict__ w, int c0, int C, int cvb) {
    for (int i = threadIdx.x; i < cvb * 8 * 9; i += blockDim.x) {
        const int ch = i / 9, t = i - ch * 9;
        const float v = (c0 + ch < C) ? w[(long)(c0 + ch) * 9 + (FLIP ? 8 - t : t)] : 0.f;
        wl[(ch >> 3) * DW_TAP_LD + t * 8 + (ch & 7)] = v;
    }
}

template <typename T, int R, bool FLIP>
__global__ __launch_bounds__(256) void k_dw3x3_strip(DwGeom g, const T* __restrict__ x, const float* __restrict__ w,
                                                     T* __restrict__ y, int accumulate, float* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    const int c0 = blockIdx.y * g.cvb * 8;
    stage_taps<FLIP>(wl, w, c0, g.C, g.cvb);
    __syncthreads();
    const int cgl = threadIdx.x % g.cvb, col = threadIdx.x / g.cvb;
    const int ch = c0 + cgl * 8;
    const bool active = col < g.ncol && ch < g.C;
    float ssum[8], ssq[8];                                   // BatchNorm batch statistics of the stored (rounded) values
#pragma unroll
    for (int j = 0; j < 8; ++j) ssum[j] = ssq[j] = 0.f;
    const __amdgpu_buffer_rsrc_t rs = buf_desc(x, g.N * g.H * g.W * g.ldx * 2);
    const float4* wq = reinterpret_cast<const float4*>(wl) + cgl;
    for (long s = blockIdx.x; active && s < g.total; s += gridDim.x) {
        const int cbk = (int)(s % g.ncb);
        const long t2 = s / g.ncb;
        const int sh = (int)(t2 % g.nsh), n = (int)(t2 / g.nsh);
        const int h0 = sh * R, wc = cbk * g.ncol + col;
        if (wc >= g.W) continue;
        u32x4 v[R + 2][3];
#pragma unroll
        for (int r = 0; r < R + 2; ++r) {
            const int hs = h0 - 1 + r;
            const bool rok = (unsigned)hs < (unsigned)g.H;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int ws = wc - 1 + c;
                const bool ok = rok && (unsigned)ws < (unsigned)g.W;
                const int off = ok ? ((((n * g.H + hs) * g.W + ws) * g.ldx + ch) * 2) : BUF_OOB;
                v[r][c] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
            }
        }
        float acc[R][8];
#pragma unroll
        for (int o = 0; o < R; ++o)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[o][j] = 0.f;
#pragma unroll
        for (int r = 0; r < R + 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float f[8];
                unpack8<T>(v[r][c], f);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int o = r - kh;
                    if (o < 0 || o >= R) continue;
                    const float4 w0 = wq[((kh * 3 + c) * 2) * g.cvb], w1 = wq[((kh * 3 + c) * 2 + 1) * g.cvb];
                    acc[o][0] = fmaf(f[0], w0.x, acc[o][0]); acc[o][1] = fmaf(f[1], w0.y, acc[o][1]);
                    acc[o][2] = fmaf(f[2], w0.z, acc[o][2]); acc[o][3] = fmaf(f[3], w0.w, acc[o][3]);
                    acc[o][4] = fmaf(f[4], w1.x, acc[o][4]); acc[o][5] = fmaf(f[5], w1.y, acc[o][5]);
                    acc[o][6] = fmaf(f[6], w1.z, acc[o][6]); acc[o][7] = fmaf(f[7], w1.w, acc[o][7]);
                }
            }
#pragma unroll
        for (int o = 0; o < R; ++o) {
            if (h0 + o >= g.H) break;
            T* dst = y + ((long)(n * g.H + h0 + o) * g.W + wc) * g.ldy + ch;
            if (!FLIP && g.bias != nullptr) {                 // folded BatchNorm (Model.fuse()): bias, then SiLU
                const float4 b0 = *reinterpret_cast<const float4*>(g.bias + ch), b1 = *reinterpret_cast<const float4*>(g.bias + ch + 4);
                acc[o][0] += b0.x; acc[o][1] += b0.y; acc[o][2] += b0.z; acc[o][3] += b0.w;
                acc[o][4] += b1.x; acc[o][5] += b1.y; acc[o][6] += b1.z; acc[o][7] += b1.w;
                if (g.act) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[o][j] = acc[o][j] * __frcp_rn(1.f + __expf(-acc[o][j]));
                }
            }
            if (accumulate) {                                 // gradient fan-in: add to what another consumer's backward left
                float prev[8];
                load_pack<T, 8>(dst, prev);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[o][j] += prev[j];
            }
            store_pack<T, 8>(dst, acc[o]);
            if (!FLIP && stats != nullptr) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float r2 = to_f<T>(from_f<T>(acc[o][j]));
                    ssum[j] += r2;
                    ssq[j] += r2 * r2;
                }
            }
        }
    }
    if (FLIP || stats == nullptr) return;
    // workgroup totals per channel (the columns of one channel group through LDS), then one atomic per channel and
    // statistic into replica (workgroup index mod 8) of the [8][2][C] accumulator -- the forward of a BatchNorm conv
    // needs no separate statistics pass over y
    __shared__ float red[256][9];
    float* o = stats + (long)(blockIdx.x & 7) * 2 * g.C;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = active ? (pass ? ssq[j] : ssum[j]) : 0.f;
        __syncthreads();
        for (int e = threadIdx.x; e < g.cvb * 8; e += 256) {
            const int cl = e >> 3, j = e & 7;
            float t = 0.f;
            for (int cc = 0; cc < g.ncol; ++cc) t += red[cc * g.cvb + cl][j];
            if (c0 + e < g.C) atomicAdd(o + pass * g.C + c0 + e, t);
        }
    }
}

// dw[c][tap] = sum_p dy[p][c] * x[p (+) tap][c].  Same strips; a thread keeps the 9 x 8 sums of its channels over all the
// strips its workgroup walks, the workgroup combines its columns through LDS one tap at a time and stores ITS partial
// [C][9] block (plain stores; k_dw_wgrad_finalize sums the workgroups).
template <typename T, int R>
__global__ __launch_bounds__(256) void k_dw3x3_wgrad_strip(DwGeom g, const T* __restrict__ x, const T* __restrict__ dy,
                                                           float* __restrict__ part) {
    __shared__ float red[256][9];
    const int c0 = blockIdx.y * g.cvb * 8;
    const int cgl = threadIdx.x % g.cvb, col = threadIdx.x / g.cvb;
    const int ch = c0 + cgl * 8;
    const bool active = col < g.ncol && ch < g.C;
    float acc[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;
    const __amdgpu_buffer_rsrc_t rsx = buf_desc(x, g.N * g.H * g.W * g.ldx * 2);
    const __amdgpu_buffer_rsrc_t rsy = buf_desc(dy, g.N * g.H * g.W * g.ldy * 2);
    if (active) {
        for (long s = blockIdx.x; s < g.total; s += gridDim.x) {
            const int cbk = (int)(s % g.ncb);
            const long t2 = s / g.ncb;
            const int sh = (int)(t2 % g.nsh), n = (int)(t2 / g.nsh);
            const int h0 = sh * R, wc = cbk * g.ncol + col;
            if (wc >= g.W) continue;
            u32x4 gv[R], v[R + 2][3];
#pragma unroll
            for (int o = 0; o < R; ++o) {
                const bool ok = h0 + o < g.H;
                gv[o] = __builtin_amdgcn_raw_buffer_load_b128(rsy, ok ? ((((n * g.H + h0 + o) * g.W + wc) * g.ldy + ch) * 2) : BUF_OOB, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < R + 2; ++r) {
                const int hs = h0 - 1 + r;
                const bool rok = (unsigned)hs < (unsigned)g.H;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int ws = wc - 1 + c;
                    const bool ok = rok && (unsigned)ws < (unsigned)g.W;
                    v[r][c] = __builtin_amdgcn_raw_buffer_load_b128(rsx, ok ? ((((n * g.H + hs) * g.W + ws) * g.ldx + ch) * 2) : BUF_OOB, 0, 0);
                }
            }
            float gf[R][8];
#pragma unroll
            for (int o = 0; o < R; ++o) unpack8<T>(gv[o], gf[o]);
#pragma unroll
            for (int r = 0; r < R + 2; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float f[8];
                    unpack8<T>(v[r][c], f);
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh) {
                        const int o = r - kh;
                        if (o < 0 || o >= R) continue;
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[kh * 3 + c][j] = fmaf(gf[o][j], f[j], acc[kh * 3 + c][j]);
                    }
                }
        }
    }
    float* pw = part + (long)blockIdx.x * g.C * 9;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = active ? acc[t][j] : 0.f;
        __syncthreads();
        for (int o = threadIdx.x; o < g.cvb * 8; o += 256) {
            const int cl = o >> 3, j = o & 7;
            float s = 0.f;
            for (int cc = 0; cc < g.ncol; ++cc) s += red[cc * g.cvb + cl][j];
            if (c0 + o < g.C) pw[(long)(c0 + o) * 9 + t] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Rows kernels.  Input row r of a band that starts at output row h0 lives in ring slot (r - h0 + 1) % D, D = DW_PF + 3:
// output row h0 + j reads slots j, j + 1, j + 2 and, before it computes, issues the loads of input row h0 + j + 1 + DW_PF
// into the slot that row h0 + j - 2 has just left.  The row loop is unrolled D times, so every slot index is static.
constexpr int DW_PF = 2;                                     // input rows in flight ahead of the row being computed
constexpr int DW_PF_WGRAD = 1;                               // weight gradient (72 sums per thread): one row less, for its three waves per SIMD

struct DwCols { unsigned off[3]; };                          // byte offset of the thread's three columns inside a row, or BUF_OOB

__device__ __forceinline__ DwCols dw_cols(int wc, int W, int ld, int ch) {
    DwCols c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ws = wc - 1 + k;
        c.off[k] = (unsigned)ws < (unsigned)W ? (unsigned)((ws * ld + ch) * 2) : (unsigned)BUF_OOB;
    }
    return c;
}

// One packet of row r of a tensor: the thread's column offset as the vector offset (a BUF_OOB column stays out of range), the
// row's offset as the scalar offset, and a descriptor of NO records for a row the caller rules out (above / below the image,
// beyond the band): zeros without a fetch, and no address arithmetic per load.
template <typename T>
__device__ __forceinline__ u32x4 dw_load(const T* p, int bytes, bool rok, unsigned coloff, unsigned rowoff) {
    const __amdgpu_buffer_rsrc_t rs = buf_desc(p, rok ? bytes : 0);
    return __builtin_amdgcn_raw_buffer_load_b128(rs, (int)coloff, (int)(rok ? rowoff : 0u), 0);
}

// the three packets of input row r of image offset imgoff (zeros above the image and beyond `rmax`, the band's lower halo row)
template <typename T>
__device__ __forceinline__ void dw_load_row(u32x4 (&v)[3], const T* p, int bytes, const DwCols& c, int r, int rmax,
                                            unsigned rowbytes, unsigned imgoff) {
    const bool rok = r >= 0 && r <= rmax;
    const unsigned rb = imgoff + (unsigned)r * rowbytes;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = dw_load<T>(p, bytes, rok, c.off[k], rb);
}

template <typename T, bool FLIP>
__global__ __launch_bounds__(256, FLIP ? 4 : 3) void k_dw3x3_rows(DwGeom g, const T* __restrict__ x, const float* __restrict__ w,
                                                    T* __restrict__ y, int accumulate, float* __restrict__ stats) {
    constexpr int D = DW_PF + 3;
    extern __shared__ __attribute__((aligned(16))) float wl[];
    const int c0 = blockIdx.y * g.cvb * 8;
    stage_taps_rows<FLIP>(wl, w, c0, g.C, g.cvb);
    __syncthreads();
    const int cgl = threadIdx.x % g.cvb, col = threadIdx.x / g.cvb;
    const int ch = c0 + cgl * 8;
    const bool active = col < g.ncol && ch < g.C;
    float ssum[8], ssq[8];                                   // BatchNorm batch statistics of the stored (rounded) values
#pragma unroll
    for (int j = 0; j < 8; ++j) ssum[j] = ssq[j] = 0.f;
    const int xbytes = g.N * g.H * g.W * g.ldx * 2;
    // what the gradient fan-in adds to is read through a descriptor too (one row ahead): no records when nothing is added
    const int ybytes = accumulate ? g.N * g.H * g.W * g.ldy * 2 : 0;
    const float4* wq = reinterpret_cast<const float4*>(wl + cgl * DW_TAP_LD);
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;   // the thread's bias, once (not per row)
    if (!FLIP && g.bias != nullptr && active) {
        b0 = *reinterpret_cast<const float4*>(g.bias + ch);
        b1 = *reinterpret_cast<const float4*>(g.bias + ch + 4);
    }
    const unsigned xrow = (unsigned)(g.W * g.ldx * 2), yrow = (unsigned)(g.W * g.ldy * 2);
    for (long s = blockIdx.x; s < g.total; s += gridDim.x) {
        const int cbk = (int)(s % g.ncb);
        const long t2 = s / g.ncb;
        const int sh = (int)(t2 % g.nsh), n = (int)(t2 / g.nsh);
        const int h0 = sh * g.hb, wc = cbk * g.ncol + col;
        if (!active || wc >= g.W) continue;
        const int h1 = h0 + g.hb < g.H ? h0 + g.hb : g.H;    // the band: output rows [h0, h1)
        const int nr = h1 - h0, rmax = h1 < g.H ? h1 : g.H - 1;
        const DwCols cx = dw_cols(wc, g.W, g.ldx, ch);
        const unsigned ximg = (unsigned)n * g.H * xrow, yimg = (unsigned)n * g.H * yrow;
        const unsigned ycol = (unsigned)((wc * g.ldy + ch) * 2);
        u32x4 v[D][3], pv[D];
#pragma unroll
        for (int i = 0; i < D - 1; ++i) dw_load_row<T>(v[i], x, xbytes, cx, h0 - 1 + i, rmax, xrow, ximg);
        pv[0] = dw_load<T>(y, ybytes, true, ycol, yimg + (unsigned)h0 * yrow);
        for (int jb = 0; jb < nr; jb += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int h = h0 + jb + u;
                if (h >= h1) break;
                asm volatile("" ::: "memory");                // per row: the taps are re-read from LDS, not kept in 72 registers
                pv[(u + 1) % D] = dw_load<T>(y, ybytes, h + 1 < h1, ycol, yimg + (unsigned)(h + 1) * yrow);
                dw_load_row<T>(v[(u + D - 1) % D], x, xbytes, cx, h + 1 + DW_PF, rmax, xrow, ximg);
                float acc[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)               // the strip kernel's order: kh outer, kw inner, from 0
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float f[8];
                        asm volatile("" : "+v"(v[(u + kh) % D][c]));   // unpacked again per row: the window stays packed (36 registers, not 72)
                        unpack8<T>(v[(u + kh) % D][c], f);
                        const float4 w0 = wq[(kh * 3 + c) * 2], w1 = wq[(kh * 3 + c) * 2 + 1];
                        acc[0] = fmaf(f[0], w0.x, acc[0]); acc[1] = fmaf(f[1], w0.y, acc[1]);
                        acc[2] = fmaf(f[2], w0.z, acc[2]); acc[3] = fmaf(f[3], w0.w, acc[3]);
                        acc[4] = fmaf(f[4], w1.x, acc[4]); acc[5] = fmaf(f[5], w1.y, acc[5]);
                        acc[6] = fmaf(f[6], w1.z, acc[6]); acc[7] = fmaf(f[7], w1.w, acc[7]);
                    }
                T* dst = y + ((long)(n * g.H + h) * g.W + wc) * g.ldy + ch;
                if (!FLIP && g.bias != nullptr) {             // folded BatchNorm (Model.fuse()): bias, then SiLU
                    acc[0] += b0.x; acc[1] += b0.y; acc[2] += b0.z; acc[3] += b0.w;
                    acc[4] += b1.x; acc[5] += b1.y; acc[6] += b1.z; acc[7] += b1.w;
                    if (g.act) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] = acc[j] * __frcp_rn(1.f + __expf(-acc[j]));
                    }
                }
                if (accumulate) {                             // gradient fan-in: add to what another consumer's backward left
                    float prev[8];
                    unpack8<T>(pv[u % D], prev);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += prev[j];
                }
                store_pack<T, 8>(dst, acc);
                if (!FLIP && stats != nullptr) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float r2 = to_f<T>(from_f<T>(acc[j]));
                        ssum[j] += r2;
                        ssq[j] += r2 * r2;
                    }
                }
            }
        }
    }
    if (FLIP || stats == nullptr) return;
    // as in the strip kernel: the thread's sums over all its bands, once per workgroup through LDS, one atomic per channel
    // and statistic into replica (workgroup index mod 8)
    __shared__ float red[256][9];
    float* o = stats + (long)(blockIdx.x & 7) * 2 * g.C;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = active ? (pass ? ssq[j] : ssum[j]) : 0.f;
        __syncthreads();
        for (int e = threadIdx.x; e < g.cvb * 8; e += blockDim.x) {
            const int cl = e >> 3, j = e & 7;
            float t = 0.f;
            for (int cc = 0; cc < g.ncol; ++cc) t += red[cc * g.cvb + cl][j];
            if (c0 + e < g.C) atomicAdd(o + pass * g.C + c0 + e, t);
        }
    }
}

// The same walk with dy(h, col) beside the window: 9 x 8 sums per thread over all the workgroup's bands, ONE combine of the
// workgroup's columns through LDS ([thread][73]: conflict-free writes) and its [C][9] partial block in plain stores.
constexpr int DW_RED_LD = 73;
constexpr size_t DW_RED_MAX = 256 * DW_RED_LD * sizeof(float);   // 73 KiB: above the default limit of dynamic LDS

template <typename T>
__global__ __launch_bounds__(256, 3) void k_dw3x3_wgrad_rows(DwGeom g, const T* __restrict__ x, const T* __restrict__ dy,
                                                          float* __restrict__ part) {
    constexpr int D = DW_PF_WGRAD + 3;
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int c0 = blockIdx.y * g.cvb * 8;
    const int cgl = threadIdx.x % g.cvb, col = threadIdx.x / g.cvb;
    const int ch = c0 + cgl * 8;
    const bool active = col < g.ncol && ch < g.C;
    float acc[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;
    const int xbytes = g.N * g.H * g.W * g.ldx * 2, ybytes = g.N * g.H * g.W * g.ldy * 2;
    const unsigned xrow = (unsigned)(g.W * g.ldx * 2), yrow = (unsigned)(g.W * g.ldy * 2);
    for (long s = blockIdx.x; s < g.total; s += gridDim.x) {
        const int cbk = (int)(s % g.ncb);
        const long t2 = s / g.ncb;
        const int sh = (int)(t2 % g.nsh), n = (int)(t2 / g.nsh);
        const int h0 = sh * g.hb, wc = cbk * g.ncol + col;
        if (!active || wc >= g.W) continue;
        const int h1 = h0 + g.hb < g.H ? h0 + g.hb : g.H;
        const int nr = h1 - h0, rmax = h1 < g.H ? h1 : g.H - 1;
        const DwCols cx = dw_cols(wc, g.W, g.ldx, ch);
        const unsigned ximg = (unsigned)n * g.H * xrow, yimg = (unsigned)n * g.H * yrow;
        const unsigned ycol = (unsigned)((wc * g.ldy + ch) * 2);
        u32x4 v[D][3], gv[D];
#pragma unroll
        for (int i = 0; i < D - 1; ++i) dw_load_row<T>(v[i], x, xbytes, cx, h0 - 1 + i, rmax, xrow, ximg);
#pragma unroll
        for (int i = 0; i <= DW_PF_WGRAD; ++i) gv[i] = dw_load<T>(dy, ybytes, h0 + i < h1, ycol, yimg + (unsigned)(h0 + i) * yrow);
        for (int jb = 0; jb < nr; jb += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int h = h0 + jb + u;
                if (h >= h1) break;
                const int hn = h + 1 + DW_PF_WGRAD;
                gv[(u + 1 + DW_PF_WGRAD) % D] = dw_load<T>(dy, ybytes, hn < h1, ycol, yimg + (unsigned)hn * yrow);
                dw_load_row<T>(v[(u + D - 1) % D], x, xbytes, cx, hn, rmax, xrow, ximg);
                float gf[8];
                unpack8<T>(gv[u % D], gf);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float f[8];
                        asm volatile("" : "+v"(v[(u + kh) % D][c]));   // unpacked again per row: the window stays packed (36 registers, not 72)
                        unpack8<T>(v[(u + kh) % D][c], f);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[kh * 3 + c][j] = fmaf(gf[j], f[j], acc[kh * 3 + c][j]);
                    }
            }
        }
    }
    const int nthr = g.cvb * g.ncol;
    if ((int)threadIdx.x < nthr) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) red[threadIdx.x * DW_RED_LD + t * 8 + j] = acc[t][j];
    }
    __syncthreads();
    float* pw = part + (long)blockIdx.x * g.C * 9;
    for (int o = threadIdx.x; o < g.cvb * 72; o += blockDim.x) {
        const int cl = o / 72, k = o - cl * 72;              // k = tap * 8 + channel of the packet
        float sum = 0.f;
        for (int cc = 0; cc < g.ncol; ++cc) sum += red[(cc * g.cvb + cl) * DW_RED_LD + k];
        const int c = c0 + cl * 8 + (k & 7);
        if (c < g.C) pw[(long)c * 9 + (k >> 3)] = sum;
    }
}

bool dw_eligible(const void* x, int ldx, const void* y, int ldy, int N, int H, int W, int C) {
    if (C % 8 || ldx % 8 || ldy % 8 || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(y) & 15)) return false;
    if ((long)N * H * W * ldx * 2 >= (1L << 31) || (long)N * H * W * ldy * 2 >= (1L << 31)) return false;
    return (long)N * H * W > 0;
}

// strip kernels: 256 / cvb columns per workgroup, strips of R rows
void dw_geom(DwGeom& g, int ldx, int ldy, int N, int H, int W, int C, int R) {
    g.N = N; g.H = H; g.W = W; g.C = C; g.ldx = ldx; g.ldy = ldy;
    const int cv = C / 8;
    g.cvb = cv < 256 ? cv : 256;
    g.ncol = 256 / g.cvb;
    if (g.ncol > W) g.ncol = W;
    g.hb = R;
    g.nsh = (H + R - 1) / R;
    g.ncb = (W + g.ncol - 1) / g.ncol;
    g.total = (long)N * g.nsh * g.ncb;
    g.bias = nullptr; g.act = 0;
}

int& dw_variant() {                                           // 0 per shape (dw_takes_rows), 1 strip, 2 rows
    static int v = [] {
        const char* e = getenv("YOLO_DW_KERNEL");
        return e == nullptr ? 0 : strcmp(e, "strip") == 0 ? 1 : strcmp(e, "rows") == 0 ? 2 : 0;
    }();
    return v;
}

}  // namespace

// The plan of the rows kernels for an (N, H, W, C) map.  Columns per workgroup: of the counts that fit 256 threads and leave
// at most a quarter of the column slots idle, the one that issues the fewest column fetches per row, ncb * (ncol + 2) (every
// column block also fetches its two halo columns), ties to the fewer idle columns.  Band height: forward / data gradient want
// at least 512 workgroups (two per CU) and every band's two halo rows cheap, so the bands are as tall as 512 workgroups
// allow; the weight gradient, whose workgroups hold 72 sums and a 73-float LDS row per thread (two workgroups per CU), wants
// at most 512, all resident at once.  Neither goes below four rows (the strip kernel's height) on a map that has them.
DwPlan dw_plan(int N, int H, int W, int C) {
    DwPlan p{};
    const int cv = C / 8;
    p.cvb = cv < 256 ? cv : 256;
    p.ncy = ceil_div(cv, p.cvb);
    const int maxcol = 256 / p.cvb < W ? 256 / p.cvb : W;
    long best = -1;
    for (int nc = 1; nc <= maxcol; ++nc) {
        const int ncb = (W + nc - 1) / nc, idle = ncb * nc - W;
        if (4 * idle > ncb * nc) continue;
        const long cost = (long)ncb * (nc + 2) * 1024 + idle;
        if (best < 0 || cost <= best) { best = cost; p.ncol = nc; p.ncb = ncb; }
    }
    p.wg = (p.cvb * p.ncol + 63) / 64 * 64;
    const long per_band = (long)N * p.ncb * p.ncy;            // workgroups of one band per image
    const int hmin = H < 4 ? H : 4;
    const long want = (512 + per_band - 1) / per_band;        // forward: at least this many bands per image ...
    p.hb = (int)(H / want) > hmin ? (int)(H / want) : hmin;
    p.nb = (H + p.hb - 1) / p.hb;
    const long most = 512 / per_band > 1 ? 512 / per_band : 1;   // ... weight gradient: at most this many
    p.hb_wg = (int)((H + most - 1) / most) > hmin ? (int)((H + most - 1) / most) : hmin;
    p.nb_wg = (H + p.hb_wg - 1) / p.hb_wg;
    const long items = (long)N * p.ncb * p.nb, items_wg = (long)N * p.ncb * p.nb_wg;
    p.grid = (int)(items < 1024 ? items : 1024);
    p.grid_wg = (int)(items_wg < 512 ? items_wg : 512);
    return p;
}

int dw_tune_set(int variant) {
    if (variant < 0 || variant > 2) return YOLO_ERR_ARG;
    dw_variant() = variant;
    return YOLO_OK;
}

// Which kernels a map takes.  Measured per shape on MI355X (tools/dw_bench.py, 32 images, bf16, graph-replayed, strip -> rows):
// forward 128 ch @80x80 27.9 -> 24.3 us and 256 ch @40x40 19.4 -> 16.5, but 128 ch @40x40 9.6 -> 11.5, 512 ch @20x20 13.0 -> 13.4
// and 128 ch @20x20 5.4 -> 6.3 (the data gradient alike): a band is a serial walk, and a map of a few megabytes is over in one
// round trip of the strip kernel's all-at-once loads.  So forward and data gradient walk rows from 16 MiB up.  The weight
// gradient walks rows everywhere: 44.8 -> 29.1, 28.3 -> 22.0, 21.3 -> 17.4, 26.6 -> 20.9, 16.4 -> 11.6 us with its finalize.
bool dw_takes_rows(int N, int H, int W, int C, bool wgrad) {
    const int v = dw_variant();
    if (v != 0) return v == 2;
    return wgrad || (long)N * H * W * C * 2 >= (16L << 20);
}

namespace {

void dw_rows_geom(DwGeom& g, const DwPlan& p, int ldx, int ldy, int N, int H, int W, int C, bool wgrad) {
    g.N = N; g.H = H; g.W = W; g.C = C; g.ldx = ldx; g.ldy = ldy;
    g.cvb = p.cvb; g.ncol = p.ncol; g.ncb = p.ncb;
    g.hb = wgrad ? p.hb_wg : p.hb;
    g.nsh = wgrad ? p.nb_wg : p.nb;
    g.total = (long)N * g.nsh * g.ncb;
    g.bias = nullptr; g.act = 0;
}

}  // namespace

// forward / data gradient; returns -1 when the tensors do not qualify (the caller falls back to the generic kernel)
int dw16_launch(bool flip, const void* x, int ldx, const float* w, void* y, int ldy, int N, int H, int W, int C, int dtype,
                int accumulate, float* stats, hipStream_t st, const float* bias, int act) {
    if (dtype != YOLO_BF16 && dtype != YOLO_F16) return -1;
    if (!dw_eligible(x, ldx, y, ldy, N, H, W, C)) return -1;
    if (bias != nullptr && (flip || stats != nullptr || (reinterpret_cast<uintptr_t>(bias) & 15))) return -1;
    DwGeom g;
    if (dw_takes_rows(N, H, W, C, false)) {
        const DwPlan p = dw_plan(N, H, W, C);
        dw_rows_geom(g, p, ldx, ldy, N, H, W, C, false);
        g.bias = bias; g.act = act;
        const dim3 grid((unsigned)p.grid, (unsigned)p.ncy);
        const size_t lds = (size_t)g.cvb * DW_TAP_LD * sizeof(float);
        static unsigned long long done[4] = {0, 0, 0, 0};
#define DW_GO(T_, FLIP_)                                                                                                        \
    do {                                                                                                                        \
        if (int rc = yolo_allow_dyn_lds(reinterpret_cast<const void*>(&k_dw3x3_rows<T_, FLIP_>), DW_TAP_MAX,                    \
                                        done[(dtype == YOLO_BF16 ? 0 : 2) + (FLIP_ ? 1 : 0)])) return rc;                       \
        hipLaunchKernelGGL((k_dw3x3_rows<T_, FLIP_>), grid, dim3(p.wg), lds, st, g, (const T_*)x, w, (T_*)y, accumulate, stats); \
    } while (0)
        if (dtype == YOLO_BF16) { if (flip) DW_GO(bf16_t, true); else DW_GO(bf16_t, false); }
        else { if (flip) DW_GO(f16_t, true); else DW_GO(f16_t, false); }
#undef DW_GO
        return YOLO_LAUNCH_CHECK();
    }
    constexpr int R = 4;
    dw_geom(g, ldx, ldy, N, H, W, C, R);
    g.bias = bias; g.act = act;
    const dim3 grid((unsigned)(g.total < 4096 ? g.total : 4096), (unsigned)ceil_div(C / 8, g.cvb));
    const size_t lds = (size_t)g.cvb * 8 * 9 * sizeof(float);
#define DW_GO(T_, FLIP_) hipLaunchKernelGGL((k_dw3x3_strip<T_, R, FLIP_>), grid, dim3(256), lds, st, g, (const T_*)x, w, (T_*)y, accumulate, stats)
    if (dtype == YOLO_BF16) { if (flip) DW_GO(bf16_t, true); else DW_GO(bf16_t, false); }
    else { if (flip) DW_GO(f16_t, true); else DW_GO(f16_t, false); }
#undef DW_GO
    return YOLO_LAUNCH_CHECK();
}

// partial: [*nrows][C][9] fp32, every entry written, *nrows <= nslab; -1 when the tensors do not qualify
int dw16_wgrad_launch(const void* x, int ldx, const void* dy, int ldy, float* partial, int nslab, int* nrows, int N, int H, int W,
                      int C, int dtype, hipStream_t st) {
    if (dtype != YOLO_BF16 && dtype != YOLO_F16) return -1;
    if (!dw_eligible(x, ldx, dy, ldy, N, H, W, C)) return -1;
    DwGeom g;
    if (dw_takes_rows(N, H, W, C, true)) {
        const DwPlan p = dw_plan(N, H, W, C);
        dw_rows_geom(g, p, ldx, ldy, N, H, W, C, true);
        *nrows = p.grid_wg < nslab ? p.grid_wg : nslab;
        const dim3 grid((unsigned)*nrows, (unsigned)p.ncy);
        const size_t lds = (size_t)g.cvb * g.ncol * DW_RED_LD * sizeof(float);
        static unsigned long long done_bf16 = 0, done_f16 = 0;
        if (dtype == YOLO_BF16) {
            if (int rc = yolo_allow_dyn_lds(reinterpret_cast<const void*>(&k_dw3x3_wgrad_rows<bf16_t>), DW_RED_MAX, done_bf16)) return rc;
            hipLaunchKernelGGL((k_dw3x3_wgrad_rows<bf16_t>), grid, dim3(p.wg), lds, st, g, (const bf16_t*)x, (const bf16_t*)dy, partial);
        } else {
            if (int rc = yolo_allow_dyn_lds(reinterpret_cast<const void*>(&k_dw3x3_wgrad_rows<f16_t>), DW_RED_MAX, done_f16)) return rc;
            hipLaunchKernelGGL((k_dw3x3_wgrad_rows<f16_t>), grid, dim3(p.wg), lds, st, g, (const f16_t*)x, (const f16_t*)dy, partial);
        }
        return YOLO_LAUNCH_CHECK();
    }
    constexpr int R = 2;
    dw_geom(g, ldx, ldy, N, H, W, C, R);
    *nrows = nslab;
    const dim3 grid((unsigned)nslab, (unsigned)ceil_div(C / 8, g.cvb));
    if (dtype == YOLO_BF16)
        hipLaunchKernelGGL((k_dw3x3_wgrad_strip<bf16_t, R>), grid, dim3(256), 0, st, g, (const bf16_t*)x, (const bf16_t*)dy, partial);
    else
        hipLaunchKernelGGL((k_dw3x3_wgrad_strip<f16_t, R>), grid, dim3(256), 0, st, g, (const f16_t*)x, (const f16_t*)dy, partial);
    return YOLO_LAUNCH_CHECK();
}
