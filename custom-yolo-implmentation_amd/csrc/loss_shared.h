// What the two loss files (loss.hip: nearest-centre assignment, loss_tal.hip: task-aligned assignment) compute the same
// way: the box decode, the per-lane softmax of one side's 16 DFL logits and the two-bin DFL cross entropy.  One copy, so the
// two losses cannot drift apart; both files are built without fma contraction, so the operation order written here is the
// order executed.
#pragma once
#include "common.h"

constexpr int LOSS_REG = 16;

// softmax expectation of the 4 x 16 DFL logits of one anchor (p: its first box logit, channel stride A) -> centre-xywh pixels
template <typename T>
__device__ __forceinline__ float4 decode_anchor(const T* __restrict__ p, long A, float ax, float ay, float st) {
    float e[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float x[LOSS_REG], mx = -INFINITY;
#pragma unroll
        for (int b = 0; b < LOSS_REG; ++b) { x[b] = to_f<T>(p[(long)(s * LOSS_REG + b) * A]); mx = fmaxf(mx, x[b]); }
        float sum = 0.f;
#pragma unroll
        for (int b = 0; b < LOSS_REG; ++b) { x[b] = expf(x[b] - mx); sum += x[b]; }
        float ex = 0.f;
#pragma unroll
        for (int b = 0; b < LOSS_REG; ++b) ex += (x[b] / sum) * (float)b;
        e[s] = ex;
    }
    float x1 = (ax - e[0]) * st, y1 = (ay - e[1]) * st, x2 = (ax + e[2]) * st, y2 = (ay + e[3]) * st;
    return make_float4((x1 + x2) / 2.f, (y1 + y2) / 2.f, x2 - x1, y2 - y1);
}

// one wave on one anchor, lane = (side, bin): softmax of the lane's side over its 16 bins from the lane's logit x
// -> p (the lane's probability), lse (the side's log-sum-exp), ev (the side's expectation)
__device__ __forceinline__ void side_softmax(float x, int bin, float& p, float& lse, float& ev) {
    float mx = x;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float ex = expf(x - mx), sum = ex;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    p = ex / sum;
    lse = mx + logf(sum);
    ev = p * (float)bin;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ev += __shfl_xor(ev, o, 64);
}

// the DFL pair of one side around the continuous target tv (clamped to [0, 14.99] here), for the lane that holds `bin`:
// contrib = the lane's share of wl (lse - x_lo) + wr (lse - x_lo+1), lx = lse - x;  gbody = p - wl [bin = lo] - wr [bin = lo + 1]
__device__ __forceinline__ void dfl_pair(float tv, int bin, float lx, float p, float& contrib, float& gbody) {
    tv = fminf(fmaxf(tv, 0.f), (float)(LOSS_REG - 1) - 0.01f);
    int lo = (int)tv;
    float wl = (float)(lo + 1) - tv, wr = tv - (float)lo;
    contrib = (bin == lo ? wl * lx : 0.f) + (bin == lo + 1 ? wr * lx : 0.f);
    gbody = p - (bin == lo ? wl : 0.f) - (bin == lo + 1 ? wr : 0.f);
}

// the 16 lanes of a side, then the four sides: every lane gets the sum over the 64
__device__ __forceinline__ float sides_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    float all = v + __shfl_xor(v, 16, 64);
    all += __shfl_xor(all, 32, 64);
    return all;
}
