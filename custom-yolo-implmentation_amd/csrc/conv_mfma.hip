// bf16 / f16 implicit-GEMM convolution on the gfx950 matrix cores (v_mfma_f32_16x16x32_{bf16,f16}).
//
// Forward and data-gradient share one kernel (ConvGeom, conv_geom.h): a 128-pixel x BN-channel
// output tile per 256-thread workgroup (4 waves), K = taps*Cs walked in 32-element steps.  The
// activation tile is gathered NHWC row by row (16 B = 8 channels per lane, zero for padding taps),
// the weight tile comes from the K-major packed matrix; both are staged through LDS (unpadded
// 64-byte rows whose four 16-byte chunks are XOR-swizzled by the row, LDSROW in conv_dev.h: conflict-free
// ds_read_b128 fragment reads) with a double buffer filled by LDS-DMA or through registers, one
// barrier per K-step.  MFMA roles are swapped (A = weights, B = activations) so a
// lane's four accumulator registers are four CONSECUTIVE output channels of one pixel: the epilogue
// stores 8 bytes per lane into NHWC rows.
//
// Weight-gradient: dW[co][tap][ci] = sum_p dY[p][co] * X[p+tap][ci].  The reduction index is the
// pixel, which is the slow axis of NHWC, so both tiles are transposed on their way into LDS
// (pixel-major inner) and the K loop runs over 32-pixel steps of one slab; slabs are combined with
// fp32 atomics into the packed gradient matrix.
#include "conv_dev.h"

namespace {

// MODE 0: K walked tap-major (k = tap*Cs + ch), any Cs % 8 == 0; each lane tracks its own (tap, ch).
// MODE 1: the same with Cs < 32 (a step can cross several taps).
// MODE 2: Cs % 32 == 0.  K is walked channel-chunk-major with the taps innermost (a workgroup re-reads its
//   input patch for all taps of one 32-channel chunk back to back, so the re-reads hit L2), the tap of a step is
//   wave-uniform, and both operands come through buffer descriptors: the per-lane byte offset (voffset) is fixed
//   for the whole loop, the step's tap / chunk / weight-column offset is one scalar (soffset), and a padding tap
//   or a row past the end is a voffset beyond the descriptor's range, which the hardware reads as zero -- the
//   gather costs 3 vector instructions per row and step.  All sizes are below 2^30 elements (host check).
// MODE 3: MODE 2 with LDS-DMA (buffer_load_dwordx4 ... lds): the tiles go global -> LDS without passing through
//   registers (no ds_write pass, 16 fewer VGPRs).  A wave instruction writes 64 x 16 B contiguously, which is exactly
//   16 rows of the swizzled 64-byte-row image when the lane in slot s of a row fetches chunk s ^ swizzle(row);
//   out-of-range lanes write zeros (tests/test_gpu_selftest.py pins both facts).
template <typename T, int WGM, int WGN, int WM, int WN, bool ACC, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_conv_mfma(GeomDev g, const T* __restrict__ src, const T* __restrict__ wm,
                                                   const float* __restrict__ bias, T* __restrict__ dst, int ntile_n) {
    static_assert(WGM * WGN == 4 && WGM * WM * 16 == BM, "tile shape");
    constexpr int BN = WGN * WN * 16;
    using ops = mfma_ops<T>;
    using frag = typename ops::frag;
    __shared__ __attribute__((aligned(16))) T lds_a[2][BM][LDSROW];
    __shared__ __attribute__((aligned(16))) T lds_b[2][BN][LDSROW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LinearTile lt = linear_tile(ntile_n);
    const int m0 = lt.tile_m * BM;
    const int cd0 = lt.tile_n * BN;
    const int total_pix = g.N * g.Hg * g.Wg;

    // ---- loader state: two activation rows (r, r+64) and up to two weight rows per thread, fixed k-segment
    const int kseg = tid & 3;
    const int lrow = tid >> 2;                      // 0..63
    const int sk = (kseg ^ ((-(lrow >> 2)) & 3)) * 8;   // swizzled chunk this thread stores
    int rowoff[2], hs0[2], ws0[2];                  // element offset of the row's (n, hs0, ws0) source pixel
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = m0 + lrow + i * 64;
        const bool rv = q < total_pix;
        const unsigned qq = rv ? q : 0;
        const unsigned t2 = qq / (unsigned)g.Wg, b = qq - t2 * g.Wg;
        const unsigned n = t2 / (unsigned)g.Hg, a = t2 - n * g.Hg;
        hs0[i] = rv ? (int)a * g.sstride : -(1 << 20);     // rows past the end fail every bounds test
        ws0[i] = (int)b * g.sstride;
        rowoff[i] = (((int)n * g.Hs + (int)a * g.sstride) * g.Ws + (int)b * g.sstride) * g.lds;
    }
    constexpr int WR = (BN + 63) / 64;              // weight rows per thread (lrow, lrow+64)
    bool wvalid[WR];
#pragma unroll
    for (int i = 0; i < WR; ++i) {
        const int r = lrow + i * 64;
        wvalid[i] = (r < BN) && (cd0 + r < g.e.Cd);
    }

    uint4 ra[2], rb[WR];

    // MODE 2 state
    unsigned vmask[2] = {0u, 0u};                   // bit t: tap t of this row is inside the source image
    int voffa[2], voffb[WR];
    int tap = 0, cbase = 0, wcol = 0;               // uniform
    __amdgpu_buffer_rsrc_t rsa, rsb;
    // MODE 0/1 state
    int ltap = 0, ch = kseg * 8;
    const T* wrow[WR];

    if constexpr (MODE >= 2) {
        for (int t = 0; t < g.ntaps; ++t) {
            const int dh = (int)((g.dh_pack >> (2 * t)) & 3u) - 1, dw = (int)((g.dw_pack >> (2 * t)) & 3u) - 1;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bool ok = (unsigned)(hs0[i] + dh) < (unsigned)g.Hs && (unsigned)(ws0[i] + dw) < (unsigned)g.Ws;
                vmask[i] |= (ok ? 1u : 0u) << t;
            }
        }
        // descriptor base = src - one row - one pixel, so the scalar tap offset (dh+1, dw+1) is never negative
        const int shift = (g.Ws + 1) * g.lds;
        rsa = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(src) - shift, 0, (g.N * g.Hs * g.Ws * g.lds + shift) * 2, BUF_FLAGS);
        rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(wm), 0, g.e.Cd * g.Kpad * 2, BUF_FLAGS);
        // register staging: this thread loads chunk kseg and stores it at the swizzled slot; LDS-DMA: the lane's
        // slot is fixed (lane-linear image), so it loads the chunk that belongs there
        const int kload = MODE == 3 ? (kseg ^ ((-(lrow >> 2)) & 3)) : kseg;
#pragma unroll
        for (int i = 0; i < 2; ++i) voffa[i] = (rowoff[i] + kload * 8) * 2;
#pragma unroll
        for (int i = 0; i < WR; ++i)
            voffb[i] = wvalid[i] ? ((cd0 + lrow + i * 64) * g.Kpad + kload * 8) * 2 : BUF_OOB;
    } else {
#pragma unroll
        for (int i = 0; i < WR; ++i) wrow[i] = wm + (long)(cd0 + (wvalid[i] ? lrow + i * 64 : 0)) * g.Kpad + kseg * 8;
        while (ch >= g.Cs) { ch -= g.Cs; ++ltap; }
    }

    auto gload = [&](int kt) {
        if constexpr (MODE >= 2) {
            const int soff = ((int)((g.dh_pack >> (2 * tap)) & 3u) * g.Ws + (int)((g.dw_pack >> (2 * tap)) & 3u)) * g.lds + cbase;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int vo = ((vmask[i] >> tap) & 1u) ? voffa[i] : BUF_OOB;
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsa, vo, soff * 2, 0);
                ra[i] = make_uint4(v.x, v.y, v.z, v.w);
            }
#pragma unroll
            for (int i = 0; i < WR; ++i) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsb, voffb[i], wcol * 2, 0);
                rb[i] = make_uint4(v.x, v.y, v.z, v.w);
            }
            if (g.tap_inner) {
                ++tap;
                wcol += g.Cs;
                if (tap == g.ntaps) { tap = 0; cbase += BK; wcol += BK - g.ntaps * g.Cs; }
            } else {
                cbase += BK;
                wcol += BK;
                if (cbase == g.Cs) { cbase = 0; ++tap; }
            }
        } else {
            const bool tv = ltap < g.ntaps;
            const int dh = (int)((g.dh_pack >> (2 * ltap)) & 3u) - 1, dw = (int)((g.dw_pack >> (2 * ltap)) & 3u) - 1;
            const int tapoff = (dh * g.Ws + dw) * g.lds + ch;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bool ok = tv && (unsigned)(hs0[i] + dh) < (unsigned)g.Hs && (unsigned)(ws0[i] + dw) < (unsigned)g.Ws;
                const uint4 v = *reinterpret_cast<const uint4*>(src + (ok ? rowoff[i] + tapoff : 0));
                ra[i] = ok ? v : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < WR; ++i) {
                const uint4 v = *reinterpret_cast<const uint4*>(wrow[i] + kt * BK);
                rb[i] = wvalid[i] ? v : make_uint4(0, 0, 0, 0);
            }
            ch += BK;
            if (MODE == 1) { while (ch >= g.Cs) { ch -= g.Cs; ++ltap; } }
            else if (ch >= g.Cs) { ch -= g.Cs; ++ltap; }
        }
    };
    // MODE 3: the same step as one LDS-DMA instruction per 16-row group (wave w: rows 16w.. and 64+16w..)
    auto gload_dma = [&](int buf) {
        const int soff = ((int)((g.dh_pack >> (2 * tap)) & 3u) * g.Ws + (int)((g.dw_pack >> (2 * tap)) & 3u)) * g.lds + cbase;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int vo = ((vmask[i] >> tap) & 1u) ? voffa[i] : BUF_OOB;
            lds_dma16(rsa, &lds_a[buf][wave * 16 + i * 64][0], vo, soff * 2);
        }
#pragma unroll
        for (int i = 0; i < WR; ++i)
            if (BN >= (i + 1) * 64 || wave * 16 + i * 64 < BN)
                lds_dma16(rsb, &lds_b[buf][wave * 16 + i * 64][0], voffb[i], wcol * 2);
        if (g.tap_inner) {
            ++tap;
            wcol += g.Cs;
            if (tap == g.ntaps) { tap = 0; cbase += BK; wcol += BK - g.ntaps * g.Cs; }
        } else {
            cbase += BK;
            wcol += BK;
            if (cbase == g.Cs) { cbase = 0; ++tap; }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            *reinterpret_cast<uint4*>(&lds_a[buf][lrow + i * 64][sk]) = ra[i];
#pragma unroll
        for (int i = 0; i < WR; ++i)
            if (BN >= (i + 1) * 64 || lrow + i * 64 < BN) *reinterpret_cast<uint4*>(&lds_b[buf][lrow + i * 64][sk]) = rb[i];
    };

    // ---- compute state
    const int wgm = wave / WGN, wgn = wave - wgm * WGN;
    const int prow = wgm * WM * 16, crow = wgn * WN * 16;
    const int fr = lane & 15;
    const int fk = ((lane >> 4) ^ ((-(fr >> 2)) & 3)) * 8;     // swizzled chunk of this lane's fragment rows
    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if constexpr (MODE == 3) {
        gload_dma(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int kt = 0; kt < g.KT; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < g.KT) gload_dma(buf ^ 1);      // the other stage was last read before the previous barrier
            frag fa[WN], fb[WM];
#pragma unroll
            for (int j = 0; j < WN; ++j) fa[j] = *reinterpret_cast<const frag*>(&lds_b[buf][crow + j * 16 + fr][fk]);
#pragma unroll
            for (int i = 0; i < WM; ++i) fb[i] = *reinterpret_cast<const frag*>(&lds_a[buf][prow + i * 16 + fr][fk]);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = ops::mma(fa[j], fb[i], acc[i][j]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    } else {
        gload(0);
        lstore(0);
        __syncthreads();
        for (int kt = 0; kt < g.KT; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < g.KT) gload(kt + 1);
            frag fa[WN], fb[WM];
#pragma unroll
            for (int j = 0; j < WN; ++j) fa[j] = *reinterpret_cast<const frag*>(&lds_b[buf][crow + j * 16 + fr][fk]);
#pragma unroll
            for (int i = 0; i < WM; ++i) fb[i] = *reinterpret_cast<const frag*>(&lds_a[buf][prow + i * 16 + fr][fk]);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = ops::mma(fa[j], fb[i], acc[i][j]);
            if (kt + 1 < g.KT) lstore(buf ^ 1);
            __syncthreads();
        }
    }

    // ---- epilogue: lane holds channels cbase..cbase+3 of pixel (tile pixel i*16 + fr)
    const int cq = (lane >> 4) * 4;
    float bv[WN][4];
    bias_blocks<WN>(bias, cd0 + crow, cq, g.e, bv);
    LinearPixels px;
    px.start(m0 + prow + fr, total_pix, g.Wg, g.Hg);
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        store_pixel_blocks<T, WN, ACC>(g.e, acc[i], bv, dst, px.pix(g.Hd, g.Wd, g.ostep, g.ooff_h, g.ooff_w), px.live(), cd0 + crow, cq, lane);
        px.advance16();
    }

    // ---- optional BatchNorm batch statistics (rows past the last pixel hold 0; LDS is idle after the K loop's last barrier)
    if (g.e.stats != nullptr)
        conv_stats_epilogue<T, WM, WN>(acc, reinterpret_cast<float*>(&lds_a[0][0][0]), BN, g.e.stats, cd0, g.e.Cd, crow, cq, fr, tid, 256);
}

// ------------------------------------------------------------------------------------------------
// weight gradient
// ------------------------------------------------------------------------------------------------
constexpr int WG_BP = 32;   // pixels per K-step
constexpr int WG_LDSROW = 40;   // 32 + 8 pad elements per LDS row

template <typename T>
__global__ __launch_bounds__(256) void k_wgrad_mfma(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int ldy,
                                                    float* __restrict__ dwp, int Kpad, int N, int H, int W, int Cin,
                                                    int OH, int OW, int Cout, int k, int stride, int ci_tiles,
                                                    long slab_pix) {
    using ops = mfma_ops<T>;
    using frag = typename ops::frag;
    __shared__ __attribute__((aligned(16))) T lds_y[64][WG_LDSROW];   // [co][pixel]
    __shared__ __attribute__((aligned(16))) T lds_x[64][WG_LDSROW];   // [ci][pixel]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int co0 = blockIdx.x * 64;
    const int tapi = blockIdx.y / ci_tiles;
    const int ci0 = (blockIdx.y - tapi * ci_tiles) * 64;
    const int kh = tapi / k, kw = tapi - kh * k, pad = k / 2;
    const long P = (long)N * OH * OW;
    const long q0 = (long)blockIdx.z * slab_pix;
    long q1 = q0 + slab_pix;
    if (q1 > P) q1 = P;
    const int steps = (int)((q1 - q0 + WG_BP - 1) / WG_BP);

    const int pix = tid & 31, seg = tid >> 5;       // 32 pixels x 8 channel segments
    const bool yv = co0 + seg * 8 < Cout, xv = ci0 + seg * 8 < Cin;

    uint4 ry, rx;
    auto gload = [&](int s) {
        long q = q0 + (long)s * WG_BP + pix;
        ry = make_uint4(0, 0, 0, 0);
        rx = make_uint4(0, 0, 0, 0);
        if (q < q1) {
            int ow = (int)(q % OW);
            long t2 = q / OW;
            int oh = (int)(t2 % OH);
            long n = t2 / OH;
            if (yv) ry = *reinterpret_cast<const uint4*>(dy + q * ldy + co0 + seg * 8);
            int ih = oh * stride + kh - pad, iw = ow * stride + kw - pad;
            if (xv && ih >= 0 && ih < H && iw >= 0 && iw < W)
                rx = *reinterpret_cast<const uint4*>(x + ((n * H + ih) * (long)W + iw) * ldx + ci0 + seg * 8);
        }
    };
    auto lstore = [&]() {
        const T* py = reinterpret_cast<const T*>(&ry);
        const T* px = reinterpret_cast<const T*>(&rx);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            lds_y[seg * 8 + j][pix] = py[j];
            lds_x[seg * 8 + j][pix] = px[j];
        }
    };

    const int wc = wave >> 1, wi = wave & 1;
    const int fr = lane & 15, fk = (lane >> 4) * 8;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (steps > 0) gload(0);
    for (int s = 0; s < steps; ++s) {
        __syncthreads();            // every wave is done reading the previous step's tiles
        lstore();
        __syncthreads();
        if (s + 1 < steps) gload(s + 1);
        frag fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const frag*>(&lds_y[wc * 32 + i * 16 + fr][fk]);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const frag*>(&lds_x[wi * 32 + j * 16 + fr][fk]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = ops::mma(fa[i], fb[j], acc[i][j]);
    }

    // D rows = co ((lane>>4)*4 + r), cols = ci (lane & 15)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int ci = ci0 + wi * 32 + j * 16 + fr;
            if (ci >= Cin) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int co = co0 + wc * 32 + i * 16 + (lane >> 4) * 4 + r;
                if (co < Cout) atomicAdd(dwp + (long)co * Kpad + tapi * Cin + ci, acc[i][j][r]);
            }
        }
}

template <typename T, int WGM, int WGN, int WM, int WN>
void launch_tile(const GeomDev& d, const void* src, const void* wm, const float* bias, void* dst, int accumulate,
                 hipStream_t st) {
    constexpr int BN = WGN * WN * 16;
    long pix = (long)d.N * d.Hg * d.Wg;
    int tm = (int)((pix + BM - 1) / BM), tn = (d.e.Cd + BN - 1) / BN;
    dim3 grid(tm * tn);
    int mode = d.Cs < BK ? 1 : (d.Cs % BK == 0 ? 2 : 0);
    if (mode == 2 && d.dma) mode = 3;
    with_acc(accumulate, [&](auto acc) {
#define CONV_LAUNCH(SM_)                                                                                              \
    hipLaunchKernelGGL((k_conv_mfma<T, WGM, WGN, WM, WN, decltype(acc)::value, SM_>), grid, dim3(256), 0, st, d,      \
                       (const T*)src, (const T*)wm, bias, (T*)dst, tn)
        if (mode == 1) CONV_LAUNCH(1); else if (mode == 2) CONV_LAUNCH(2); else if (mode == 3) CONV_LAUNCH(3); else CONV_LAUNCH(0);
#undef CONV_LAUNCH
    });
}

template <typename T>
void launch_conv_t(const GeomDev& d_in, int bn, const void* src, const void* wm, const float* bias, void* dst, int accumulate,
                   hipStream_t st) {
    GeomDev d = d_in;
    const ConvTune& tu = conv_tune();
    if (tu.tap_inner >= 0) d.tap_inner = tu.tap_inner;
    if (tu.dma >= 0) d.dma = tu.dma;
    if (bn == 128) launch_tile<T, 2, 2, 4, 4>(d, src, wm, bias, dst, accumulate, st);        // 128 x 128
    else if (bn == 64) launch_tile<T, 2, 2, 4, 2>(d, src, wm, bias, dst, accumulate, st);    // 128 x 64
    else launch_tile<T, 4, 1, 2, 2>(d, src, wm, bias, dst, accumulate, st);                  // 128 x 32
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

static int& wide_state() {
    static int v = [] { const char* e = getenv("YOLO_CONV_WIDE"); const int m = e ? atoi(e) : 2; return m < 0 ? 0 : m > 2 ? 2 : m; }();
    return v;
}
int conv_wide_flag() { return wide_state(); }
// test / A-B override of the 16-byte epilogue stores (store_pixel_blocks): 0 off, 1 exchange through ds_bpermute, 2 exchange
// through v_permlane16_swap
extern "C" int yolo_conv_wide_set(int on) { wide_state() = on < 0 ? 0 : on > 2 ? 2 : on; return YOLO_OK; }

// What the MFMA families (this file, conv_halo / conv_ring / conv_rows.hip) share: addressing and alignment
int mfma_conv_addressable(const ConvGeom& g, int dtype, const void* src, const void* wm, const void* dst) {
    if (dtype != YOLO_BF16 && dtype != YOLO_F16) return 0;
    if (g.lds % 8 || g.Cd % 8 || g.ldd % 4) return 0;
    // 32-bit byte offsets / buffer descriptors in the gather, 32-bit pixel indices
    if (!desc_addressable((long)g.N * g.Hs * g.Ws * g.lds + (long)(g.Ws + 1) * g.lds)) return 0;
    if (!pixels_addressable((long)g.N * g.Hg * g.Wg + 256)) return 0;       // up to the end of the last pixel tile
    if (!al16(src) || !al16(wm) || (reinterpret_cast<uintptr_t>(dst) & 7)) return 0;
    for (int t = 0; t < g.ntaps; ++t)
        if (g.dh[t] < -1 || g.dh[t] > 1 || g.dw[t] < -1 || g.dw[t] > 1) return 0;
    return 1;
}

// Shapes with an MFMA kernel at all (the gather kernel takes every one of them; which family runs: conv_select.hip)
int mfma_conv_eligible(const ConvGeom& g, int dtype, const void* src, const void* wm, const void* dst) {
    return mfma_conv_addressable(g, dtype, src, wm, dst) && g.Cs % 8 == 0 && desc_addressable((long)g.Cd * g.Kpad);
}

// the gather kernel with a bn-channel tile (32 / 64 / 128)
int mfma_conv_launch(const ConvGeom& g, int bn, const void* src, const void* wm, const float* bias, void* dst, int accumulate,
                     int dtype, hipStream_t st) {
    GeomDev d = to_dev(g);
    if (dtype == YOLO_BF16) launch_conv_t<bf16_t>(d, bn, src, wm, bias, dst, accumulate, st);
    else launch_conv_t<f16_t>(d, bn, src, wm, bias, dst, accumulate, st);
    return YOLO_LAUNCH_CHECK();
}

int mfma_wgrad_eligible(int Cin, int Cout, int ldx, int ldy, int dtype, const void* x, const void* dy) {
    if (dtype != YOLO_BF16 && dtype != YOLO_F16) return 0;
    if (Cin % 8 || Cout % 8 || ldx % 8 || ldy % 8) return 0;
    return al16(x) && al16(dy);
}

int mfma_wgrad_launch(const void* x, int ldx, const void* dy, int ldy, float* dwp, int Kpad, int N, int H, int W,
                      int Cin, int OH, int OW, int Cout, int k, int stride, int dtype, hipStream_t st) {
    long P = (long)N * OH * OW;
    if (P == 0) return YOLO_OK;
    int cot = (Cout + 63) / 64, cit = (Cin + 63) / 64, nt = k * k;
    long tiles = (long)cot * cit * nt;
    long max_slabs = 4096 / tiles;
    if (max_slabs < 1) max_slabs = 1;
    long slab = (P + max_slabs - 1) / max_slabs;
    if (slab < 1024) slab = 1024;
    slab = (slab + WG_BP - 1) / WG_BP * WG_BP;
    int nslab = (int)((P + slab - 1) / slab);
    dim3 grid(cot, cit * nt, nslab);
    if (dtype == YOLO_BF16)
        hipLaunchKernelGGL((k_wgrad_mfma<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, ldx, (const bf16_t*)dy, ldy,
                           dwp, Kpad, N, H, W, Cin, OH, OW, Cout, k, stride, cit, slab);
    else
        hipLaunchKernelGGL((k_wgrad_mfma<f16_t>), grid, dim3(256), 0, st, (const f16_t*)x, ldx, (const f16_t*)dy, ldy,
                           dwp, Kpad, N, H, W, Cin, OH, OW, Cout, k, stride, cit, slab);
    return YOLO_LAUNCH_CHECK();
}
