// Device-side pieces shared by the MFMA conv kernels (conv_mfma / conv_ring / conv_rows / conv_halo / conv_up2.hip and the
// fused stem of stem.hip): MFMA wrappers, the packed geometry passed by value, and the ONE copy of the kernels' tail -- bias
// gather, linear pixel walk, pixel store (ConvEpi, store_pixel_blocks) and the BatchNorm statistics epilogue
// (conv_stats_epilogue) -- plus the accumulate dispatch (with_acc).  Ring idiom and tile decode: conv_stage.h.
#pragma once
#include <cstdlib>
#include "conv_host.h"
#include "conv_stage.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

template <typename T> struct mfma_ops;
template <> struct mfma_ops<bf16_t> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct mfma_ops<f16_t> {
    typedef f16x8 frag;
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

constexpr int BM = 128;    // destination pixels per workgroup
constexpr int BK = 32;     // K elements per step (one MFMA K)
constexpr int LDSROW = 32; // elements per LDS row: THE 64-byte-row image, unpadded rows whose four 16-byte chunks are XOR-swizzled
                           // by (-(row >> 2)) & 3 -- conflict-free for ds_read_b128 fragment reads (16 rows x 1 chunk per lane
                           // group) and for ds_write_b128 staging (2 rows x 4 chunks per 8 lanes); 16 rows = one LDS-DMA piece

// What the kernels' shared tail reads, declared once and embedded in every family's kernarg struct (to_epi fills it)
struct ConvEpi {
    int Cd, ldd;                 // destination channels and row stride
    int act;                     // inference epilogue: 1 = SiLU after the bias
    int ldr, ld2;                // row strides of res / acc2
    int wide;                    // 16-byte epilogue stores where the destination allows (YOLO_CONV_WIDE=0: the 8-byte form, A/B runs)
    const void* res;             // inference epilogue: residual added after the activation (row stride ldr) or null
    const void* acc2;            // ACC launches: second accumulate source (row stride ld2) or null
    float* stats;                // optional [8][2][Cd] batch-statistics accumulator (forward of a BN conv)
};

struct GeomDev {           // ConvGeom with the tap offsets packed (no dynamic indexing of kernargs)
    int N, Hs, Ws, Cs, lds, Hd, Wd, Hg, Wg, ostep, ooff_h, ooff_w, sstride, ntaps, KT, Kpad;
    unsigned dh_pack, dw_pack;   // 2 bits per tap: value + 1
    int tap_inner;               // MODE 2 K order: 1 = taps innermost, 0 = channel chunks innermost
    int dma;                     // MODE 2 -> 3: tiles go global -> LDS by LDS-DMA instead of through registers
    ConvEpi e;
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// LDS-DMA as the BUILTIN, which hipcc sees and waits for by itself (the ring kernels use lds_dma_piece, conv_stage.h): 16 bytes
// per lane from a descriptor into LDS at dst + 16*lane (wave-uniform dst).  Wrapped: the host pass must not see the builtin.
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rs, void* dst, int voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, voffset, soffset, 0, 0);
#endif
}

// x + (x rotated by N lanes inside its row of 16): one VALU op (v_add_f32 with a DPP operand)
template <int N> __device__ __forceinline__ float row_ror_add(float x) {
    return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xf, 0xf, true));
}
__device__ __forceinline__ float row16_sum(float x) {
    x = row_ror_add<8>(x);
    x = row_ror_add<4>(x);
    x = row_ror_add<2>(x);
    return row_ror_add<1>(x);
}


// the inference epilogue on one group of four channels: v = act(v) (+ residual)
template <typename T>
__device__ __forceinline__ void fused_epilogue(float (&v)[4], int act, const void* res, long off) {
    if (act) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] * __frcp_rn(1.f + __expf(-v[r]));
    }
    if (res != nullptr) {
        float o[4];
        load_pack<T, 4>((const T*)res + off, o);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += o[r];
    }
}

// value of lane ^ 16 (gfx950's v_permlane16_swap_b32 swaps the odd 16-lane rows of its first operand with the even rows of
// its second: with both operands = v, the first result holds v[lane - 16] in the odd rows, the second v[lane + 16] in the even
// rows; tests/test_gpu_selftest.py pins the mapping)
__device__ __forceinline__ unsigned swap_rows16(unsigned v, bool odd_row) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return odd_row ? r[0] : r[1];
}

// Epilogue of one output pixel: the WN 16-channel blocks of accumulator row `a` (lane: channels cq .. cq+3 of every block,
// pixel = the lane's fr) -> bias, inference act / residual, accumulate sources, store.  Shared by the five MFMA conv kernels.
// 16-byte stores where the destination allows it (base 16-byte aligned, row stride a multiple of 8 channels, ConvEpi::wide): lanes
// (fr, fg) and (fr, fg ^ 1) hold neighbouring channel quads of the SAME pixel for every block j; one dword pair swapped
// between them (lane ^ 16) leaves the even lane with 8 consecutive channels of block j and the odd lane with 8 of block j+1 --
// half as many, twice as wide write requests per wave instruction (same-box A/B on the step with k_conv_mfma alone:
// 10.51 -> 10.38 ms; 512 -> 128 @80x80 data gradient 97 -> 78 us).  EVERY lane of the wave must call this (`live` false
// for pixels outside the map): the exchange is a cross-lane operation.
template <typename T, int WN, bool ACC>
__device__ __forceinline__ void store_pixel_blocks(const ConvEpi& g, const f32x4 (&a)[WN], const float (&bv)[WN][4], T* __restrict__ dst,
                                                   long pix, bool live, int cbase, int cq, int lane) {
    T* drow = dst + pix * g.ldd;
    auto values = [&](int j, float (&v)[4]) {
        const int c = cbase + j * 16 + cq;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = a[j][r] + bv[j][r];
        if (!live || c >= g.Cd) return;
        if (g.act | (g.res != nullptr)) fused_epilogue<T>(v, g.act, g.res, pix * g.ldr + c);
        if (ACC) {
            float o[4];
            load_pack<T, 4>(drow + c, o);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += o[r];
            if (g.acc2 != nullptr) {
                load_pack<T, 4>((const T*)g.acc2 + pix * g.ld2 + c, o);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += o[r];
            }
        }
    };
    const bool wide = sizeof(T) == 2 && (WN % 2 == 0) && g.wide && ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) && (g.ldd % 8 == 0);
    if (wide) {
        const bool odd = (lane >> 4) & 1;
#pragma unroll
        for (int j = 0; j + 1 < WN; j += 2) {
            float va[4], vb[4];
            values(j, va);
            values(j + 1, vb);
            pack_t<T, 4> pa, pb;
#pragma unroll
            for (int r = 0; r < 4; ++r) { pa.v[r] = from_f<T>(va[r]); pb.v[r] = from_f<T>(vb[r]); }
            const uint2 ua = __builtin_bit_cast(uint2, pa), ub = __builtin_bit_cast(uint2, pb);
            const uint2 send = odd ? ua : ub;                      // what the partner keeps
            uint2 recv;
            if (g.wide == 2) {                                     // v_permlane16_swap: a VALU exchange of 16-lane rows, no LDS op
                recv.x = swap_rows16(send.x, odd);
                recv.y = swap_rows16(send.y, odd);
            } else {
                recv.x = __shfl_xor(send.x, 16, 64);
                recv.y = __shfl_xor(send.y, 16, 64);
            }
            // even lane: block j, channels cq .. cq+7 = own | partner's; odd lane: block j+1, channels cq-4 .. cq+3
            const uint4 out = odd ? make_uint4(recv.x, recv.y, ub.x, ub.y) : make_uint4(ua.x, ua.y, recv.x, recv.y);
            const int c8 = cbase + (odd ? j + 1 : j) * 16 + (odd ? cq - 4 : cq);
            if (live && c8 < g.Cd) *reinterpret_cast<uint4*>(drow + c8) = out;
        }
    } else if (live) {
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int c = cbase + j * 16 + cq;
            if (c >= g.Cd) continue;            // Cd % 8 == 0 => a group of 4 is all-in or all-out
            float v[4];
            values(j, v);
            store_pack<T, 4>(drow + c, v);
        }
    }
}

// bias of the lane's four channels in each of its WN 16-channel blocks (channels cbase + j*16 + cq ..+3); 0 without a bias
// and past the last channel.  Cd is read from the record HERE, not passed by value: handed in as a value it is loaded at the
// call and k_conv_halo, k_conv_ring and the accumulating k_conv_mfma allocate 1-12 more VGPRs (one halo tile loses a wave).
template <int WN>
__device__ __forceinline__ void bias_blocks(const float* __restrict__ bias, int cbase, int cq, const ConvEpi& e, float (&bv)[WN][4]) {
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int c = cbase + j * 16 + cq;
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[j][r] = (bias != nullptr && c < e.Cd) ? bias[c + r] : 0.f;
    }
}

// Epilogue walk of the kernels whose tile is a run of the linear pixel index of an Hg x Wg grid: the first pixel's
// coordinates come from two divisions, the following ones (+16 pixels each) by carrying.
struct LinearPixels {
    int q, npix, Wg, Hg, n, a, b;
    __device__ __forceinline__ void start(int q0, int npix_, int Wg_, int Hg_) {
        q = q0; npix = npix_; Wg = Wg_; Hg = Hg_;
        const unsigned qq = q < npix ? q : 0;
        const unsigned t2 = qq / (unsigned)Wg;
        b = (int)(qq - t2 * Wg);
        n = (int)(t2 / (unsigned)Hg);
        a = (int)t2 - n * Hg;
    }
    __device__ __forceinline__ bool live() const { return q < npix; }
    // destination pixel index of grid pixel (n, a, b); 0 for a dead pixel
    __device__ __forceinline__ long pix(int Hd, int Wd, int ostep, int ooff_h, int ooff_w) const {
        return live() ? ((long)n * Hd + a * ostep + ooff_h) * (long)Wd + b * ostep + ooff_w : 0;
    }
    __device__ __forceinline__ void advance16() {
        q += 16;
        b += 16;
        while (b >= Wg) {
            b -= Wg;
            if (++a == Hg) { a = 0; ++n; }
        }
    }
};

// ---- BatchNorm batch statistics of the values just stored: per-channel sum / sum of squares, no second pass over y.
// sacc = [2][BN] floats of LDS.
__device__ __forceinline__ void stats_zero(float* sacc, int n, int tid, int nthr) {
    for (int t = tid; t < n; t += nthr) sacc[t] = 0.f;
}
// the lane's accumulators rounded to T (the stored values), summed over its WM pixels and then over the 16 pixels of the
// lane row; the fr == 0 lanes add the row's sums to sacc
template <typename T, int WM, int WN>
__device__ __forceinline__ void stats_lane_sums(const f32x4 (&acc)[WM][WN], float* sacc, int BN, int crow, int cq, int fr) {
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        float s[4] = {0.f, 0.f, 0.f, 0.f}, q2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = to_f<T>(from_f<T>(acc[i][j][r]));
                s[r] += v;
                q2[r] += v * v;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = row16_sum(s[r]);
            q2[r] = row16_sum(q2[r]);
        }
        if (fr == 0) {
            const int cl = crow + j * 16 + cq;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                atomicAdd(&sacc[cl + r], s[r]);
                atomicAdd(&sacc[BN + cl + r], q2[r]);
            }
        }
    }
}
// the workgroup's sums -> replica (workgroup mod 8) of stats[8][2][Cd]
__device__ __forceinline__ void stats_flush(const float* sacc, int BN, float* stats, int cd0, int Cd, int tid, int nthr) {
    float* o = stats + (long)(blockIdx.x & 7) * 2 * Cd;
    for (int t = tid; t < BN; t += nthr)
        if (cd0 + t < Cd) {
            atomicAdd(o + cd0 + t, sacc[t]);
            atomicAdd(o + Cd + cd0 + t, sacc[BN + t]);
        }
}
// The statistics epilogue of a conv kernel whose workgroup (nthr threads) owns channels cd0 .. cd0+BN-1; acc[i][j] = the
// lane's pixel tile i, 16-channel block j (channels crow + j*16 + cq ..+3 of the tile).  The contract:
//   * ALL threads of the workgroup call it (two barriers inside);
//   * LDS is idle at the call: sacc may alias what the K loop used, so every wave is past its last LDS read and no LDS-DMA
//     is in flight (the caller's barrier, where its K loop does not end in one);
//   * acc rows of dead pixels (outside the map, past the last pixel) hold 0;
//   * acc is the raw conv result: no bias (a launch has a bias or statistics, not both), rounded here as the store rounds it;
//   * the sums are ADDED to replica blockIdx.x & 7 of stats[8][2][Cd]: the consumer sums all eight.
template <typename T, int WM, int WN>
__device__ __forceinline__ void conv_stats_epilogue(const f32x4 (&acc)[WM][WN], float* sacc, int BN, float* stats, int cd0, int Cd,
                                                    int crow, int cq, int fr, int tid, int nthr) {
    stats_zero(sacc, 2 * BN, tid, nthr);
    __syncthreads();
    stats_lane_sums<T, WM, WN>(acc, sacc, BN, crow, cq, fr);
    __syncthreads();
    stats_flush(sacc, BN, stats, cd0, Cd, tid, nthr);
}

// ---- host side
inline ConvEpi to_epi(const ConvGeom& g) {
    ConvEpi e;
    e.Cd = g.Cd; e.ldd = g.ldd; e.act = g.act; e.ldr = g.ldr; e.ld2 = g.ld2;
    e.wide = conv_wide_flag();
    e.res = g.res; e.acc2 = g.acc2; e.stats = g.stats;
    return e;
}

inline GeomDev to_dev(const ConvGeom& g) {
    GeomDev d;
    d.N = g.N; d.Hs = g.Hs; d.Ws = g.Ws; d.Cs = g.Cs; d.lds = g.lds; d.Hd = g.Hd; d.Wd = g.Wd;
    d.Hg = g.Hg; d.Wg = g.Wg; d.ostep = g.ostep; d.ooff_h = g.ooff_h; d.ooff_w = g.ooff_w;
    d.sstride = g.sstride; d.ntaps = g.ntaps; d.Kpad = g.Kpad; d.KT = g.Kpad / BK;
    pack_taps(g, &d.dh_pack, &d.dw_pack);
    d.tap_inner = 0;
    d.dma = 1;      // LDS-DMA staging: level or a few % ahead of register staging on every shape of tools/conv_tune.py
    d.e = to_epi(g);
    return d;
}

// f(std::true_type / std::false_type): the ACC template argument of a kernel from the launch's run-time flag
template <typename F>
decltype(auto) with_acc(int accumulate, F&& f) {
    if (accumulate) return f(std::bool_constant<true>{});
    return f(std::bool_constant<false>{});
}

}  // namespace
