// The front half the MFMA conv kernels share: the LDS-DMA piece with its counted wait (the ring idiom), the
// ring kernel's row swizzle and the workgroup -> tile decode.  Only what leaves every kernel's device code as it was lives
// here: descriptor, swizzle, lds-base, ring-slot and stage-row helpers each re-ordered the kernels' address arithmetic under
// hipcc, so those stay written out, with the flags word and the out-of-range offset by name (common.h).
#pragma once
#include <type_traits>
#include "common.h"

namespace {

template <int I> using ic = std::integral_constant<int, I>;       // a compile-time step index handed to a generic lambda

// ---- LDS-DMA ring
// One piece: 64 lanes x 16 bytes from the descriptor (voffset per lane + scalar offset) to LDS at lds_addr + 16*lane.
// M0, the LDS destination base, is written in the SAME asm statement that reads it: the compiler reserves M0 and does not
// preserve it from one statement to the next, and an "m0" clobber only draws a warning.
// Being inline asm, the load is invisible to hipcc's wait insertion; the kernels count the queue themselves (dma_wait).
// lds_dma16 (conv_dev.h) stays for the gather kernel's MODE 3: that builtin IS visible to hipcc, which then waits vmcnt(0)
// before the step's first LDS read by itself, and k_conv_mfma's double buffer relies on exactly that.
__device__ __forceinline__ void lds_dma_piece(__amdgpu_buffer_rsrc_t rs, unsigned lds_addr, int voff, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :: "s"(lds_addr), "v"(voff), "s"(rs), "s"(soff) : "memory");
}
// The counted wait in front of a step's barrier (all but this wave's N youngest pieces have landed; N is each kernel's own
// proof and stays at its call site) ALSO waits for this wave's own LDS reads (lgkmcnt(0)): the barrier declares the stage
// read in the previous step free, and hipcc software-pipelines fragment reads across a raw s_barrier (the reads are issued
// before it, their s_waitcnt lgkmcnt comes after it).  A refill that has to fetch from memory arrives long after such a read
// has executed; the pieces issued past the end of K through a descriptor of zero records (they keep the count the same in
// every iteration) fetch nothing and can land first -- the read then returns zeros: one (chunk, tap) product missing from a
// whole workgroup tile, sporadically (found in k_dgrad2_patch: DESIGN section 6; tools/dbg_up2.py).
// That barrier is a raw __builtin_amdgcn_s_barrier(), never __syncthreads(): a piece in flight is a pending LDS write on
// the VM counter, so the fence of __syncthreads() emits vmcnt(0) and drains the ring at every step.
template <int N> __device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(N) : "memory"); }

// Chunk swizzle of the ring kernel's LDS rows, applied to the lane's SOURCE chunk (a DMA image is lane-linear): slot s of row
// r holds chunk s ^ swz(r).  RB = bytes per row: 128 (64-deep steps, eight chunks) or 64 (the image at LDSROW, conv_dev.h)
template <int RB> __device__ __forceinline__ int lds_swz(int row) {
    if constexpr (RB == 128) return (row >> 1) & 7;
    else return (-(row >> 2)) & 3;
}

// ---- workgroup -> tile
// bijective XCD-aware remap (guide T1): blocks that share an XCD get a contiguous range of tiles
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}
// (pixel tile, channel tile), channel tiles innermost.  k_conv_ring keeps its own two lines: this function changed its code.
struct LinearTile { int tile_m, tile_n; };
__device__ __forceinline__ LinearTile linear_tile(int ntile_n) {
    const int tile = xcd_remap(blockIdx.x, gridDim.x), tile_m = tile / ntile_n;
    return {tile_m, tile - tile_m * ntile_n};
}
// kernels whose pixel tile is a TH x TW block of one image: image n, block origin (y0, x0), first channel cd0
struct BlockTile { int n, y0, x0, cd0, tile_n; };
template <int TH, int TW, int BN> __device__ __forceinline__ BlockTile block_tile(int tiles_h, int tiles_w, int ntile_n) {
    const LinearTile l = linear_tile(ntile_n);
    const int per_img = tiles_h * tiles_w;
    const int n = l.tile_m / per_img, trem = l.tile_m - n * per_img;
    const int ty = trem / tiles_w, tx = trem - ty * tiles_w;
    return {n, ty * TH, tx * TW, l.tile_n * BN, l.tile_n};
}

}  // namespace
