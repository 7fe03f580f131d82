// bf16 / f16 implicit-GEMM convolution (forward and data gradient) with a software-pipelined LDS ring.
//
// k_conv_mfma (conv_mfma.hip) issues the next K-step's tiles, then waits for ALL of them before it reads the current
// ones: hipcc cannot tell which LDS bytes a `buffer_load ... lds` builtin writes, so it puts `s_waitcnt vmcnt(0)` in
// front of the first ds_read of every step -- inside one workgroup nothing overlaps, and layers with one workgroup per
// CU or fewer (every 20x20 / 40x40 map of the model) run at one L2 round trip per 32-deep K-step.  Here:
//   * K-steps of 64 elements (two MFMA k-blocks per barrier, LDS rows of 128 bytes = one full cache line per pixel row
//     and step, the eight 16-byte chunks of a row XOR-swizzled by (row >> 1) & 7) or of 32 elements (the 64-byte-row
//     image, LDSROW in conv_dev.h): conflict-free ds_read_b128 fragment reads; the swizzle (lds_swz, conv_stage.h) is
//     applied to the lane's SOURCE chunk, the LDS-DMA image is lane-linear;
//   * a ring of NST stages filled by LDS-DMA issued from inline asm (invisible to hipcc's wait insertion) and retired
//     by a COUNTED wait for all but (NST-2) * loads per stage + one raw s_barrier per step: NST-1 steps of loads
//     stay in flight across barriers.  Stages past the end of K are issued with out-of-range offsets (the hardware
//     writes zeros, no memory traffic), so the count is the same in every iteration.  This is the ring idiom; its one
//     copy -- lds_dma_piece, dma_wait and the hazards they carry -- is conv_stage.h;
//   * both operands through buffer descriptors as in k_conv_mfma: fixed per-lane byte offset, one scalar offset per
//     step (tap, channel chunk), padding taps / rows past the end / partial channel chunks = offset out of range = 0;
//   * up to four sub-problems per launch (the four parity classes of a stride-2 data gradient: own tap list, weight
//     matrix and destination phase) -- one launch of ~4x the workgroups instead of four small ones.
// Source channels: a multiple of 32, at least 64 (narrower layers stay on k_conv_mfma).  MFMA roles are swapped
// (A = weights, B = activations): a lane's four accumulator registers are four consecutive output channels.
#include "conv_dev.h"

namespace {

struct RingSub {
    int Hg, Wg, ooff_h, ooff_w, ntaps, KT, Kpad, wm_off, tile0, npix;
    unsigned dh_pack, dw_pack;
};
struct RingGeom {
    int N, Hs, Ws, Cs, lds, Hd, Wd, ostep, sstride, nsub, spt, ntile_n, wm_elems;
    ConvEpi e;
    RingSub sub[4];
};

// RB = bytes per LDS row = bytes of K per step: 128 (64-deep steps, 8 rows per piece) or 64 (32-deep steps, 16 rows per piece)
template <typename T, int RB, int WGM, int WGN, int WM, int WN, int NST, bool ACC>
__global__ __launch_bounds__(256) void k_conv_ring(RingGeom g, const T* __restrict__ src, const T* __restrict__ wm,
                                                   const float* __restrict__ bias, T* __restrict__ dst) {
    static_assert(WGM * WGN == 4 && (RB == 64 || RB == 128), "four waves; 32- or 64-deep steps");
    constexpr int BM_ = WGM * WM * 16, BN = WGN * WN * 16;
    constexpr int KE = RB / 2, SLOTS = RB / 16, RPP = 64 / SLOTS;     // K elements per step; 16-byte chunks per row; rows per piece
    constexpr int LA = BM_ / (4 * RPP), LB = BN / (4 * RPP);          // LDS-DMA pieces per wave and stage
    static_assert(LA >= 1 && LB >= 1 && BM_ % (4 * RPP) == 0 && BN % (4 * RPP) == 0, "tile shape");
    constexpr int L = LA + LB;
    constexpr int A_BYTES = BM_ * RB, STAGE = (BM_ + BN) * RB;
    using ops = mfma_ops<T>;
    using frag = typename ops::frag;
    __shared__ __attribute__((aligned(1024))) char smem[NST * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = tile / g.ntile_n, tile_n = tile - tile_m * g.ntile_n;
    int cls = 0;
    for (int i = 1; i < g.nsub; ++i)
        if (tile_m >= g.sub[i].tile0) cls = i;
    const RingSub sb = g.sub[cls];
    const int m0 = (tile_m - sb.tile0) * BM_;
    const int cd0 = tile_n * BN;

    // ---- loader state.  Wave w fills rows [w*BM/4, (w+1)*BM/4) of the activation tile and [w*BN/4, ...) of the weight
    // tile, RPP rows per piece: lane = (row in piece) * SLOTS + slot, and the chunk that belongs in slot s of row r is
    // s ^ swz(r).  A row past the last pixel / channel gets an out-of-range offset once and for all.
    const int rp = lane / SLOTS, slot = lane % SLOTS;
    int voffa[LA], voffb[LB];
    unsigned vmask[LA];                                       // bit t: tap t of this row is inside the source image
    unsigned tailok = 0;                                      // bit i / bit 8+j: the lane's chunk exists in a partial last chunk step
    const int spt = (g.Cs + KE - 1) / KE;                     // steps per tap
    const int tail_c0 = (spt - 1) * KE;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int row = wave * (BM_ / 4) + i * RPP + rp;
        const int chunk = slot ^ lds_swz<RB>(row);
        const int q = m0 + row;
        const bool rv = q < sb.npix;
        const unsigned qq = rv ? q : 0;
        const unsigned t2 = qq / (unsigned)sb.Wg, b = qq - t2 * sb.Wg;
        const unsigned n = t2 / (unsigned)sb.Hg, a = t2 - n * sb.Hg;
        const int hs0 = (int)a * g.sstride, ws0 = (int)b * g.sstride;
        voffa[i] = rv ? ((((int)n * g.Hs + hs0) * g.Ws + ws0) * g.lds + chunk * 8) * 2 : BUF_OOB;
        unsigned m = 0;
        for (int t = 0; t < sb.ntaps; ++t) {
            const int dh = (int)((sb.dh_pack >> (2 * t)) & 3u) - 1, dw = (int)((sb.dw_pack >> (2 * t)) & 3u) - 1;
            const bool ok = (unsigned)(hs0 + dh) < (unsigned)g.Hs && (unsigned)(ws0 + dw) < (unsigned)g.Ws;
            m |= (ok ? 1u : 0u) << t;
        }
        vmask[i] = m;
        tailok |= (tail_c0 + chunk * 8 < g.Cs ? 1u : 0u) << i;
    }
#pragma unroll
    for (int j = 0; j < LB; ++j) {
        const int row = wave * (BN / 4) + j * RPP + rp;
        const int chunk = slot ^ lds_swz<RB>(row);
        voffb[j] = (cd0 + row < g.e.Cd) ? (sb.wm_off + (cd0 + row) * sb.Kpad + chunk * 8) * 2 : BUF_OOB;
        tailok |= (tail_c0 + chunk * 8 < g.Cs ? 1u : 0u) << (8 + j);
    }
    // descriptor base = src - one row - one pixel, so the scalar tap offset (dh+1, dw+1) is never negative
    const int shift = (g.Ws + 1) * g.lds;
    const int a_bytes = (g.N * g.Hs * g.Ws * g.lds + shift) * 2, w_bytes = g.wm_elems * 2;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
    const bool partial = (g.Cs % KE) != 0;
    const bool taps = sb.ntaps > 1;                           // a one-tap conv has no padding taps: nothing per lane and step

    int tap = 0, cstep = 0, issued = 0, wbuf = 0;             // uniform: the step the next issue() fetches
    auto issue = [&]() {
        const bool live = issued < sb.KT;                     // past the end of K: zero records, nothing fetched, same piece count
        const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(src) - shift, 0, live ? a_bytes : 0, BUF_FLAGS);
        const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(wm), 0, live ? w_bytes : 0, BUF_FLAGS);
        const int t = live ? tap : 0;
        const int soffa = (((int)((sb.dh_pack >> (2 * t)) & 3u) * g.Ws + (int)((sb.dw_pack >> (2 * t)) & 3u)) * g.lds + cstep * KE) * 2;
        const int soffb = (t * g.Cs + cstep * KE) * 2;
        const unsigned base = lds0 + wbuf * STAGE + wave * (LA * 1024);
        const unsigned baseb = lds0 + wbuf * STAGE + A_BYTES + wave * (LB * 1024);
        if (partial && cstep == spt - 1) {                    // last chunk step of a tap, channel count not a multiple of the step
#pragma unroll
            for (int i = 0; i < LA; ++i) {
                const bool ok = ((vmask[i] >> t) & 1u) && ((tailok >> i) & 1u);
                lds_dma_piece(rsa, base + i * 1024, ok ? voffa[i] : BUF_OOB, soffa);
            }
#pragma unroll
            for (int j = 0; j < LB; ++j) lds_dma_piece(rsb, baseb + j * 1024, ((tailok >> (8 + j)) & 1u) ? voffb[j] : BUF_OOB, soffb);
        } else if (taps) {
            const unsigned bit = 1u << t;
#pragma unroll
            for (int i = 0; i < LA; ++i) lds_dma_piece(rsa, base + i * 1024, (vmask[i] & bit) ? voffa[i] : BUF_OOB, soffa);
#pragma unroll
            for (int j = 0; j < LB; ++j) lds_dma_piece(rsb, baseb + j * 1024, voffb[j], soffb);
        } else {
#pragma unroll
            for (int i = 0; i < LA; ++i) lds_dma_piece(rsa, base + i * 1024, voffa[i], soffa);
#pragma unroll
            for (int j = 0; j < LB; ++j) lds_dma_piece(rsb, baseb + j * 1024, voffb[j], soffb);
        }
        ++issued;
        if (++cstep == spt) { cstep = 0; ++tap; }
        if (++wbuf == NST) wbuf = 0;
    };

    // ---- compute state
    const int wgm = wave / WGN, wgn = wave - wgm * WGN;
    const int prow = wgm * WM * 16, crow = wgn * WN * 16;
    const int fr = lane & 15, fg = lane >> 4;
    const int fsw = lds_swz<RB>(fr);                         // swizzle of this lane's fragment rows (row bases are multiples of 16)
    const int foff0 = fr * RB + ((fg ^ fsw) * 16), foff1 = fr * RB + (((4 + fg) ^ fsw) * 16);
    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < NST - 1; ++s) issue();
    int rbuf = 0;
    for (int kt = 0; kt < sb.KT; ++kt) {
        dma_wait<(NST - 2) * L>();                            // this wave's pieces of stage kt have landed ...
        __builtin_amdgcn_s_barrier();                         // ... and so have everyone else's; stage kt-1 is free again
        issue();                                              // refill the stage read in the previous step
        const char* sa = smem + rbuf * STAGE + prow * RB;
        const char* sw = smem + rbuf * STAGE + A_BYTES + crow * RB;
#pragma unroll
        for (int ks = 0; ks < RB / 64; ++ks) {
            const int fo = ks ? foff1 : foff0;
            frag fa[WN], fb[WM];
#pragma unroll
            for (int j = 0; j < WN; ++j) fa[j] = *reinterpret_cast<const frag*>(sw + j * (16 * RB) + fo);
#pragma unroll
            for (int i = 0; i < WM; ++i) fb[i] = *reinterpret_cast<const frag*>(sa + i * (16 * RB) + fo);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = ops::mma(fa[j], fb[i], acc[i][j]);
        }
        if (++rbuf == NST) rbuf = 0;
    }
    dma_wait<0>();                                            // the zero-fill pieces issued past the end of K

    // ---- epilogue: lane holds channels c..c+3 of pixel (tile pixel prow + i*16 + fr)
    const int cq = fg * 4;
    float bv[WN][4];
    bias_blocks<WN>(bias, cd0 + crow, cq, g.e, bv);
    LinearPixels px;
    px.start(m0 + prow + fr, sb.npix, sb.Wg, sb.Hg);
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        store_pixel_blocks<T, WN, ACC>(g.e, acc[i], bv, dst, px.pix(g.Hd, g.Wd, g.ostep, sb.ooff_h, sb.ooff_w), px.live(), cd0 + crow, cq, lane);
        px.advance16();
    }

    // ---- optional BatchNorm batch statistics (rows past the last pixel hold 0)
    if (g.e.stats != nullptr) {
        __builtin_amdgcn_s_barrier();                         // every wave is past its last fragment read and its DMA drain
        conv_stats_epilogue<T, WM, WN>(acc, reinterpret_cast<float*>(smem), BN, g.e.stats, cd0, g.e.Cd, crow, cq, fr, tid, 256);
    }
}

template <typename T, int RB, int WGM, int WGN, int WM, int WN, int NST>
void launch_ring_t(const RingGeom& g, int nwg, const void* src, const void* wm, const float* bias, void* dst, int accumulate,
                   hipStream_t st) {
    with_acc(accumulate, [&](auto acc) {
        hipLaunchKernelGGL((k_conv_ring<T, RB, WGM, WGN, WM, WN, NST, decltype(acc)::value>), dim3(nwg), dim3(256), 0, st, g,
                           (const T*)src, (const T*)wm, bias, (T*)dst);
    });
}

template <typename T>
int launch_ring(const RingGeom& g, const RingTile& t, int nwg, const void* src, const void* wm, const float* bias, void* dst,
                int accumulate, hipStream_t st) {
#define RING_CASE(BK__, BM__, BN__, NST__, WGM_, WGN_, WM_, WN_)                                                      \
    if (t.bk == BK__ && t.bm == BM__ && t.bn == BN__ && t.nst == NST__) {                                             \
        launch_ring_t<T, 2 * BK__, WGM_, WGN_, WM_, WN_, NST__>(g, nwg, src, wm, bias, dst, accumulate, st);          \
        return YOLO_LAUNCH_CHECK();                                                                                   \
    }
#define RING_DEPTHS(BK__, BM__, BN__, WGM_, WGN_, WM_, WN_)                                                           \
    RING_CASE(BK__, BM__, BN__, 2, WGM_, WGN_, WM_, WN_)                                                              \
    RING_CASE(BK__, BM__, BN__, 3, WGM_, WGN_, WM_, WN_)                                                              \
    RING_CASE(BK__, BM__, BN__, 4, WGM_, WGN_, WM_, WN_)
    RING_DEPTHS(64, 128, 128, 2, 2, 4, 4)
    RING_DEPTHS(64, 128, 64, 2, 2, 4, 2)
    RING_DEPTHS(64, 64, 128, 2, 2, 2, 4)
    RING_DEPTHS(64, 64, 64, 2, 2, 2, 2)
    RING_DEPTHS(64, 128, 32, 4, 1, 2, 2)
    RING_DEPTHS(32, 128, 128, 2, 2, 4, 4)
    RING_DEPTHS(32, 128, 64, 2, 2, 4, 2)
    RING_DEPTHS(32, 64, 128, 2, 2, 2, 4)
    RING_DEPTHS(32, 64, 64, 2, 2, 2, 2)
#undef RING_DEPTHS
#undef RING_CASE
    return YOLO_ERR_ARG;
}

}  // namespace

// Shapes the ring kernel can run (where it is USED: conv_select.hip): what the MFMA families share, source channels a
// multiple of 32 and at least 64, and a weight matrix the kernel's byte offsets reach.  The factor 4: one launch may carry
// the four parity classes of a stride-2 data gradient, whose matrices lie in ONE buffer under one descriptor (wm_off), and
// together they are no larger than four times this one.
int ring_conv_eligible(const ConvGeom& g, int dtype, const void* src, const void* wm, const void* dst) {
    return mfma_conv_addressable(g, dtype, src, wm, dst) && g.Cs % 32 == 0 && g.Cs >= 64 && desc_addressable((long)g.Cd * g.Kpad * 4);
}

// gs[0..n): sub-problems that share source, destination tensor, channel counts and strides (n = 1, or the four parity
// classes of a stride-2 data gradient; empty classes are skipped); wm_off[c] = element offset of class c's packed
// weight matrix inside wm, wm_elems = size of the whole buffer
int ring_conv_launch(const ConvGeom* gs, int n, const RingTile& t, const long* wm_off, long wm_elems, const void* src,
                     const void* wm, const float* bias, void* dst, int accumulate, int dtype, hipStream_t st) {
    if (n < 1 || n > 4 || !desc_addressable(wm_elems)) return YOLO_ERR_ARG;
    const ConvGeom& g0 = gs[0];
    RingGeom d;
    d.N = g0.N; d.Hs = g0.Hs; d.Ws = g0.Ws; d.Cs = g0.Cs; d.lds = g0.lds; d.Hd = g0.Hd; d.Wd = g0.Wd;
    d.ostep = g0.ostep; d.sstride = g0.sstride;
    d.e = to_epi(g0);
    d.spt = (g0.Cs + t.bk - 1) / t.bk;
    d.ntile_n = (g0.Cd + t.bn - 1) / t.bn;
    d.wm_elems = (int)wm_elems;
    d.nsub = 0;
    int tiles = 0;
    for (int c = 0; c < n; ++c) {
        const ConvGeom& g = gs[c];
        const long npix = (long)g.N * g.Hg * g.Wg;
        if (npix == 0) continue;
        RingSub& s = d.sub[d.nsub++];
        s.Hg = g.Hg; s.Wg = g.Wg; s.ooff_h = g.ooff_h; s.ooff_w = g.ooff_w; s.ntaps = g.ntaps; s.KT = g.ntaps * d.spt; s.Kpad = g.Kpad;
        s.wm_off = (int)wm_off[c]; s.tile0 = tiles; s.npix = (int)npix;
        pack_taps(g, &s.dh_pack, &s.dw_pack);
        tiles += (int)((npix + t.bm - 1) / t.bm);
    }
    if (d.nsub == 0) return YOLO_OK;
    for (int c = d.nsub; c < 4; ++c) d.sub[c] = d.sub[0];
    const int nwg = tiles * d.ntile_n;
    if (dtype == YOLO_BF16) return launch_ring<bf16_t>(d, t, nwg, src, wm, bias, dst, accumulate, st);
    return launch_ring<f16_t>(d, t, nwg, src, wm, bias, dst, accumulate, st);
}
