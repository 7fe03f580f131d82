// YoloTALoss forward + gradient: task-aligned assignment (top-k anchors per GT by s^alpha iou^beta), CIoU box term, soft
// class targets normalised by their sum, DFL weighted by the target score (DESIGN 4.5 has the definition).
//
//   preds  [N][64+nc][A]  (T, anchor index fastest)  ->  out[4] = {total, box (CIoU), cls (BCE), dfl} (fp32)
//                                                        dpreds [N][64+nc][A] (T) = d total / d preds [* grad_scale]
// SIX launches (two of them one block), no host synchronisation, every grid sized by the row CAPACITY G (the live count is
// gt_off[N], read on the device; rows past it do nothing):
//   k_tal_decode  : per (n, a) the shared box decode -> pbox; clears the owner word; the per-anchor (label, t) word starts
//                   as "no target" (-1), or "poisoned" (-2) where the decoded box is not finite.
//   k_tal_topk    : one block of four waves per GT row (one wave per row scanned 8400 anchors alone: 129 us, the longest
//                   launch; the scan is latency-bound, so the four waves share it).  ONE scan of the image's anchors, four
//                   per lane in flight; a candidate (centre strictly inside the GT, finite box) gets its metric and goes
//                   into the lane's sorted list of KMAX entries (registers, fully unrolled, no dynamic index).  Then `topk`
//                   rounds of an arg-max over the 256 lane heads (butterfly per wave, the four waves through LDS; larger
//                   metric, then lower anchor); the winning lane pops.  Every chosen (anchor, align, iou) goes to the GT's
//                   list and bids for the anchor with an integer atomicMax on (iou bits, ~row): order-independent, the
//                   larger IoU and then the lower row wins.
//   k_tal_resolve : one wave per GT row, one lane per list entry: which entries it still owns, ma = max align, mi = max
//                   iou over those (a max is exact in any order), t = align mi / (ma + 1e-9) into the anchor's (label, t)
//                   word, the row's sum of t by a fixed butterfly.
//   k_tal_tss     : one block: the rows' sums in a fixed order, tss = max(sum, 1).
//   k_tal_final   : heterogeneous grid.  Blocks [0, nblk): BCE-with-logits of every class logit against the looked-up
//                   target (one (label, t) load per anchor packet serves eight classes), value partials per block, the
//                   gradient (s - t) lambda_cls / tss written once.  Blocks [nblk, nblk + FB): the 64 box-logit gradients
//                   of every anchor that is not a positive: 0, or NaN where the box is poisoned.  Blocks after those: one
//                   wave per (GT row, list entry), lane = (side, bin): CIoU and DFL of an owned entry, value and the 64
//                   gradients.
//   k_tal_finish  : one block: the class partials and the per-entry box / DFL values in a fixed order -> out[4].
// The two one-block launches replace "the last block to take a ticket sums": that needs an agent-scope release in every
// block, which on this chip writes back the XCD's L2 -- measured 567 us for k_tal_final with it (3737 blocks, each just
// having dirtied its share of dpreds) against a kernel boundary of under 2 us.
// No float atomics anywhere: two runs give the same bits.  fp32 arithmetic without fma contraction (build.py NO_CONTRACT).
#include "common.h"
#include "loss_shared.h"

namespace {

constexpr int REG = LOSS_REG;
constexpr int KMAX = 16;                 // list entries per GT: topk <= KMAX
constexpr int DENSE_BLOCKS = 2048;
constexpr int FILL_BLOCKS = 1024;
constexpr int CH = 8;                    // classes (dense) / box channels (fill) per work item
constexpr float EPS7 = 1e-7f, EPS9 = 1e-9f;
constexpr float KV = 0.40528473456935109f;   // 4 / pi^2
constexpr int NO_TARGET = -1, POISONED = -2;

struct TalDims {
    int N, A, nc, G, topk;
    float alpha, beta, lambda_box, lambda_cls, lambda_dfl;
};

struct TalWs {
    float4* pbox;                // [N A]   centre-xywh pixels
    unsigned long long* owner;   // [N A]   (iou bits << 32) | ~row of the winning bid, 0: nobody
    int2* tl;                    // [N A]   (label | NO_TARGET | POISONED, t bits)
    int* la;                     // [G KMAX] chosen anchors of a row, best first
    float* lal;                  // [G KMAX] their align
    float* lio;                  // [G KMAX] their iou
    float* ebox;                 // [G KMAX] t (1 - ciou) of an owned entry, else 0
    float* edfl;                 // [G KMAX] t dfl
    int* cnt;                    // [G]     entries in the row's list
    float* gma;                  // [G]     max align over the owned entries (-1: none)
    float* gmi;                  // [G]     max iou
    float* gts;                  // [G]     sum of t
    double* partial;             // [DENSE_BLOCKS]
    float* tss;                  // [1]
    size_t bytes;
};

static inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }

static TalWs carve(void* base, int N, int A, int G) {
    const size_t na = (size_t)N * A, g = (size_t)(G > 0 ? G : 1);
    char* p = (char*)base;
    TalWs w;
    auto take = [&](size_t b) { char* q = p; p += up16(b); return q; };
    w.pbox = (float4*)take(na * 16);
    w.owner = (unsigned long long*)take(na * 8);
    w.tl = (int2*)take(na * 8);
    w.la = (int*)take(g * KMAX * 4);
    w.lal = (float*)take(g * KMAX * 4);
    w.lio = (float*)take(g * KMAX * 4);
    w.ebox = (float*)take(g * KMAX * 4);
    w.edfl = (float*)take(g * KMAX * 4);
    w.cnt = (int*)take(g * 4);
    w.gma = (float*)take(g * 4);
    w.gmi = (float*)take(g * 4);
    w.gts = (float*)take(g * 4);
    w.partial = (double*)take((size_t)DENSE_BLOCKS * 8);
    w.tss = (float*)take(16);
    w.bytes = (size_t)(p - (char*)base);
    return w;
}

__device__ __forceinline__ bool finite_(float v) { return fabsf(v) < INFINITY; }      // false for NaN
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// x^p for x >= 0 as exp(p log x); x = 0 gives 0 (1 for p = 0), NaN stays NaN
__device__ __forceinline__ float powp(float x, float p) {
    if (x > 0.f) return expf(p * logf(x));
    return x == 0.f ? (p == 0.f ? 1.f : 0.f) : NAN;
}

__device__ __forceinline__ int live_rows(const int* __restrict__ gt_off, int N, int G) {
    const int l = gt_off[N];
    return l < G ? l : G;
}

// the GT row as the kernels use it: corners, label, image; ok = false for a row that must do nothing (label or image out of
// range, NaN included: no index is ever formed from such a value)
struct GtRow {
    float x1, y1, x2, y2;
    int cls, n;
    bool ok;
};
__device__ __forceinline__ GtRow load_gt(const float* __restrict__ gt, const int* __restrict__ gt_img, int j, int N, int nc) {
    const float* g = gt + (long)j * 5;
    const float gx = g[0], gy = g[1], gw = g[2], gh = g[3], gc = g[4];
    GtRow r;
    r.x1 = gx - gw / 2.f, r.y1 = gy - gh / 2.f, r.x2 = gx + gw / 2.f, r.y2 = gy + gh / 2.f;
    r.n = gt_img[j];
    r.ok = r.n >= 0 && r.n < N && gc >= 0.f && gc < (float)nc;
    r.cls = r.ok ? (int)gc : 0;
    if (!r.ok) r.n = 0;
    return r;
}

__device__ __forceinline__ void corners_of(const float4& pb, float& X1, float& Y1, float& X2, float& Y2) {
    X1 = pb.x - pb.z / 2.f, Y1 = pb.y - pb.w / 2.f, X2 = pb.x + pb.z / 2.f, Y2 = pb.y + pb.w / 2.f;
}

// the metric's IoU: intersection clamped at 0, denominator w1 h1 + w2 h2 - inter + 1e-7
__device__ __forceinline__ float plain_iou(const float4& pb, const GtRow& g) {
    float X1, Y1, X2, Y2;
    corners_of(pb, X1, Y1, X2, Y2);
    const float iw = fmaxf(fminf(X2, g.x2) - fmaxf(X1, g.x1), 0.f), ih = fmaxf(fminf(Y2, g.y2) - fmaxf(Y1, g.y1), 0.f);
    const float inter = iw * ih;
    const float den = (X2 - X1) * (Y2 - Y1) + (g.x2 - g.x1) * (g.y2 - g.y1) - inter + EPS7;
    return inter / den;
}

template <typename T>
__global__ __launch_bounds__(256) void k_tal_decode(TalDims d, const T* __restrict__ preds, const T* __restrict__ anchors,
                                                    const T* __restrict__ strides, TalWs w) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)d.N * d.A) return;
    const int a = (int)(i % d.A);
    const long n = i / d.A;
    const T* p = preds + n * (long)(4 * REG + d.nc) * d.A + a;
    const float4 b = decode_anchor<T>(p, d.A, to_f<T>(anchors[a]), to_f<T>(anchors[d.A + a]), to_f<T>(strides[a]));
    w.pbox[i] = b;
    w.owner[i] = 0ull;
    const bool fin = finite_(b.x) && finite_(b.y) && finite_(b.z) && finite_(b.w);
    w.tl[i] = make_int2(fin ? NO_TARGET : POISONED, 0);
}

template <typename T>
__global__ __launch_bounds__(256) void k_tal_topk(TalDims d, const T* __restrict__ preds, const T* __restrict__ anchors,
                                                  const T* __restrict__ strides, const float* __restrict__ gt,
                                                  const int* __restrict__ gt_img, const int* __restrict__ gt_off, TalWs w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = blockIdx.x;
    if (j >= live_rows(gt_off, d.N, d.G)) return;             // block-uniform, like every return below
    const GtRow g = load_gt(gt, gt_img, j, d.N, d.nc);
    if (!g.ok) {
        if (threadIdx.x == 0) w.cnt[j] = 0;
        return;
    }
    const float4* pb = w.pbox + (long)g.n * d.A;
    const T* xc = preds + ((long)g.n * (4 * REG + d.nc) + 4 * REG + g.cls) * d.A;
    float L[KMAX], LI[KMAX];
    int LA[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; ++i) L[i] = -1.f, LI[i] = 0.f, LA[i] = 0x7fffffff;

    auto inside = [&](float ax, float ay, float st) {
        const float px = ax * st, py = ay * st;
        return px - g.x1 > EPS9 && py - g.y1 > EPS9 && g.x2 - px > EPS9 && g.y2 - py > EPS9;
    };
    auto insert = [&](int a, const float4& b, float x) {
        if (!(finite_(b.x) && finite_(b.y) && finite_(b.z) && finite_(b.w))) return;
        float io = plain_iou(b, g);
        float v = powp(sigm(x), d.alpha) * powp(io, d.beta);  // NaN: every comparison below is false
        int ai = a;
        bool moved = false;
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {                      // sorted insert: a later equal goes behind the earlier ones
            if (moved ? v >= L[i] : v > L[i]) {
                const float tv = L[i], ti = LI[i];
                const int ta = LA[i];
                L[i] = v, LI[i] = io, LA[i] = ai;
                v = tv, io = ti, ai = ta;
                moved = true;
            }
        }
    };
    // the four waves interleave 64-anchor stretches (a GT's candidates are runs of neighbouring anchors: this balances them);
    // four anchors per lane in flight, considered in index order
    int a = wave * 64 + lane;
    for (; a + 3 * 256 < d.A; a += 4 * 256) {
        bool c[4];
        float4 b[4];
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            c[u] = inside(to_f<T>(anchors[a + u * 256]), to_f<T>(anchors[d.A + a + u * 256]), to_f<T>(strides[a + u * 256]));
#pragma unroll
        for (int u = 0; u < 4; ++u) {                         // the candidates' boxes and logits: all loads before the first use
            b[u] = c[u] ? pb[a + u * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
            x[u] = c[u] ? to_f<T>(xc[a + u * 256]) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c[u]) insert(a + u * 256, b[u], x[u]);
    }
    for (; a < d.A; a += 256)
        if (inside(to_f<T>(anchors[a]), to_f<T>(anchors[d.A + a]), to_f<T>(strides[a]))) insert(a, pb[a], to_f<T>(xc[a]));

    // `topk` rounds: arg-max over the lane heads of each wave (butterfly), then over the four waves through LDS (two buffers
    // in turn: one barrier per round); larger align, then lower anchor
    __shared__ float sv[2][4], si[2][4];
    __shared__ int sa[2][4];
    int count = 0;
    for (int r = 0; r < d.topk; ++r) {
        float hv = L[0], hi = LI[0];
        int ha = LA[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(hv, o, 64), oi = __shfl_xor(hi, o, 64);
            const int oa = __shfl_xor(ha, o, 64);
            if (ov > hv || (ov == hv && oa < ha)) hv = ov, hi = oi, ha = oa;
        }
        const int buf = r & 1;
        if (lane == 0) sv[buf][wave] = hv, si[buf][wave] = hi, sa[buf][wave] = ha;
        __syncthreads();
        hv = sv[buf][0], hi = si[buf][0], ha = sa[buf][0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (sv[buf][q] > hv || (sv[buf][q] == hv && sa[buf][q] < ha)) hv = sv[buf][q], hi = si[buf][q], ha = sa[buf][q];
        if (hv < 0.f) break;                                  // every list is empty (block-uniform)
        if (threadIdx.x == 0) {
            w.la[j * KMAX + r] = ha, w.lal[j * KMAX + r] = hv, w.lio[j * KMAX + r] = hi;
            const unsigned long long key = ((unsigned long long)__float_as_uint(hi) << 32) | (unsigned long long)(0xffffffffu - (unsigned)j);
            atomicMax(w.owner + (long)g.n * d.A + ha, key);
        }
        if (LA[0] == ha) {                                    // an anchor sits in one lane of one wave only: that lane pops
#pragma unroll
            for (int i = 0; i + 1 < KMAX; ++i) L[i] = L[i + 1], LI[i] = LI[i + 1], LA[i] = LA[i + 1];
            L[KMAX - 1] = -1.f, LI[KMAX - 1] = 0.f, LA[KMAX - 1] = 0x7fffffff;
        }
        ++count;
    }
    if (threadIdx.x == 0) w.cnt[j] = count;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_tal_resolve(TalDims d, const float* __restrict__ gt, const int* __restrict__ gt_img,
                                                     const int* __restrict__ gt_off, TalWs w) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int live = live_rows(gt_off, d.N, d.G);
    if (j < live) {
        const GtRow g = load_gt(gt, gt_img, j, d.N, d.nc);
        const int c = w.cnt[j];
        const bool mine = lane < c;                           // c = 0 for a row that is not ok
        const int a = mine ? w.la[j * KMAX + lane] : 0;
        const long slot = (long)g.n * d.A + a;
        const bool owned = mine && (unsigned)(w.owner[slot] & 0xffffffffull) == 0xffffffffu - (unsigned)j;
        const float al = owned ? w.lal[j * KMAX + lane] : -1.f, io = owned ? w.lio[j * KMAX + lane] : -1.f;
        float ma = al, mi = io;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) ma = fmaxf(ma, __shfl_xor(ma, o, 64)), mi = fmaxf(mi, __shfl_xor(mi, o, 64));
        const float t = owned ? al * mi / (ma + EPS9) : 0.f;
        if (owned) w.tl[slot] = make_int2(g.cls, __float_as_int(t));
        float ts = t;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) ts += __shfl_xor(ts, o, 64);
        if (lane == 0) w.gma[j] = ma, w.gmi[j] = mi, w.gts[j] = ts;
    }
}

// one block: threads take the rows strided, a fixed butterfly per wave, the four waves in order
__global__ __launch_bounds__(256) void k_tal_tss(TalDims d, const int* __restrict__ gt_off, TalWs w) {
    __shared__ float red[4];
    const int live = live_rows(gt_off, d.N, d.G);
    float s = 0.f;
    for (int r = threadIdx.x; r < live; r += 256) s += w.gts[r];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *w.tss = fmaxf((red[0] + red[1]) + (red[2] + red[3]), 1.f);
}

// ---- the dense class pass: work item = (image, packet of V anchors, chunk of CH classes)
template <typename T, int V>
__device__ __forceinline__ void dense_part(const TalDims& d, int block, int nblk, const T* __restrict__ preds, T* __restrict__ dpreds,
                                           const TalWs& w, float coef) {
    __shared__ float red[4];
    const int AP = d.A / V, NCH = (d.nc + CH - 1) / CH;
    const long items = (long)d.N * NCH * AP, per_img = (long)(4 * REG + d.nc) * d.A;
    float lsum = 0.f;
    for (long it = block * 256L + threadIdx.x; it < items; it += nblk * 256L) {
        const int ap = (int)(it % AP);
        const long rest = it / AP;
        const int cc = (int)(rest % NCH), n = (int)(rest / NCH);
        const int c0 = cc * CH, cn = d.nc - c0 < CH ? d.nc - c0 : CH;
        const long base = n * per_img + (long)(4 * REG + c0) * d.A + (long)ap * V;
        pack_t<T, V> raw[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) raw[u] = load_raw<T, V>(preds + base + (long)(u < cn ? u : 0) * d.A);
        int lab[V];
        float tt[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int2 q = w.tl[(long)n * d.A + ap * V + e];
            lab[e] = q.x, tt[e] = __int_as_float(q.y);
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            if (u >= cn) break;
            float x[V], gr[V];
            unpack<T, V>(raw[u], x);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float t = lab[e] == c0 + u ? tt[e] : 0.f;
                const float ab = fabsf(x[e]), ex = expf(-ab), den = 1.f + ex;
                lsum += fmaxf(x[e], 0.f) - x[e] * t + log1pf(ex);
                const float s = x[e] >= 0.f ? 1.f / den : ex / den;
                gr[e] = ab < INFINITY ? (s - t) * coef : NAN;            // a NaN or infinite logit never gives a finite gradient
            }
            if (dpreds) store_pack<T, V>(dpreds + base + (long)u * d.A, gr);
        }
    }
    lsum = wave_sum(lsum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) w.partial[block] = (double)red[0] + red[1] + red[2] + red[3];
}

// ---- box logits of the anchors that are not positives: work item = (image, packet of V anchors, chunk of CH channels)
template <typename T, int V>
__device__ __forceinline__ void fill_part(const TalDims& d, int block, int fblk, T* __restrict__ dpreds, const TalWs& w) {
    const int AP = d.A / V, NCH = 4 * REG / CH;
    const long items = (long)d.N * NCH * AP, per_img = (long)(4 * REG + d.nc) * d.A;
    for (long it = block * 256L + threadIdx.x; it < items; it += fblk * 256L) {
        const int ap = (int)(it % AP);
        const long rest = it / AP;
        const int cc = (int)(rest % NCH), n = (int)(rest / NCH);
        T* out = dpreds + n * per_img + (long)(cc * CH) * d.A + (long)ap * V;
        int lab[V];
        bool plain = true;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            lab[e] = w.tl[(long)n * d.A + ap * V + e].x;
            plain &= lab[e] == NO_TARGET;
        }
        if (plain) {
            float z[V];
#pragma unroll
            for (int e = 0; e < V; ++e) z[e] = 0.f;
#pragma unroll
            for (int u = 0; u < CH; ++u) store_pack<T, V>(out + (long)u * d.A, z);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (lab[e] >= 0) continue;                    // a positive: its wave writes the 64
                const T v = from_f<T>(lab[e] == POISONED ? NAN : 0.f);
#pragma unroll
                for (int u = 0; u < CH; ++u) out[(long)u * d.A + e] = v;
            }
        }
    }
}

// CIoU of (pb, g) and d ciou / d (X1, Y1, X2, Y2); alpha_v is a constant of the gradient.  min / max split a tie evenly and
// clamp(min = 0) passes the gradient at >= 0, as ATen does.
__device__ __forceinline__ float lt_half(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float ciou_terms(const float4& pb, const GtRow& g, float (&dc)[4]) {
    float X1, Y1, X2, Y2;
    corners_of(pb, X1, Y1, X2, Y2);
    const float w1 = X2 - X1, h1 = (Y2 - Y1) + EPS7, w2 = g.x2 - g.x1, h2 = (g.y2 - g.y1) + EPS7;
    const float iwr = fminf(X2, g.x2) - fmaxf(X1, g.x1), ihr = fminf(Y2, g.y2) - fmaxf(Y1, g.y1);
    const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
    const float inter = iw * ih;
    const float uni = w1 * h1 + w2 * h2 - inter + EPS7;
    const float iou = inter / uni;
    const float cw = fmaxf(X2, g.x2) - fminf(X1, g.x1), ch = fmaxf(Y2, g.y2) - fminf(Y1, g.y1);
    const float c2 = cw * cw + ch * ch + EPS7;
    const float sx = (g.x1 + g.x2) - (X1 + X2), sy = (g.y1 + g.y2) - (Y1 + Y2);
    const float rho2 = (sx * sx + sy * sy) / 4.f;
    const float da = atanf(w2 / h2) - atanf(w1 / h1);
    const float v = KV * da * da;
    const float av = v / (v - iou + 1.f + EPS7);
    const float pen = rho2 / c2;
    // ---- d / d (X1, Y1, X2, Y2)
    const float pw = iwr >= 0.f ? 1.f : 0.f, ph = ihr >= 0.f ? 1.f : 0.f;
    const float dI[4] = {-ih * pw * lt_half(g.x1, X1), -iw * ph * lt_half(g.y1, Y1), ih * pw * lt_half(X2, g.x2), iw * ph * lt_half(Y2, g.y2)};
    const float dA[4] = {-h1, -w1, h1, w1};
    const float kA = inter / (uni * uni), kI = 1.f / uni + kA;
    const float dC[4] = {-2.f * cw * lt_half(X1, g.x1), -2.f * ch * lt_half(Y1, g.y1), 2.f * cw * lt_half(g.x2, X2), 2.f * ch * lt_half(g.y2, Y2)};
    const float dR[4] = {-sx / 2.f, -sy / 2.f, -sx / 2.f, -sy / 2.f};
    const float kP = rho2 / (c2 * c2);
    const float kv = -2.f * KV * da / (w1 * w1 + h1 * h1);
    const float dV[4] = {-kv * h1, kv * w1, kv * h1, -kv * w1};
#pragma unroll
    for (int k = 0; k < 4; ++k) dc[k] = (kI * dI[k] - kA * dA[k]) - (dR[k] / c2 - kP * dC[k]) - av * dV[k];
    return iou - (pen + v * av);
}

// ---- the positives: one wave per (row, list entry); lane = (side, bin) of the 64 box logits
template <typename T>
__device__ __forceinline__ void positive_part(const TalDims& d, int q, const T* __restrict__ preds, T* __restrict__ dpreds,
                                              const T* __restrict__ anchors, const T* __restrict__ strides, const float* __restrict__ gt,
                                              const int* __restrict__ gt_img, const int* __restrict__ gt_off, const TalWs& w, float gsc) {
    const int lane = threadIdx.x & 63, j = q >> 2, r = ((q & 3) << 2) + (threadIdx.x >> 6);
    if (j >= live_rows(gt_off, d.N, d.G)) return;
    const GtRow g = load_gt(gt, gt_img, j, d.N, d.nc);
    const bool mine = r < w.cnt[j];
    const int a = mine ? w.la[j * KMAX + r] : 0;
    const long slot = (long)g.n * d.A + a;
    const bool owned = mine && (unsigned)(w.owner[slot] & 0xffffffffull) == 0xffffffffu - (unsigned)j;
    if (!owned) {                                             // wave-uniform
        if (lane == 0) w.ebox[j * KMAX + r] = 0.f, w.edfl[j * KMAX + r] = 0.f;
        return;
    }
    const float t = __int_as_float(w.tl[slot].y), tss = *w.tss;
    const int side = lane >> 4, bin = lane & 15;
    const long per_img = (long)(4 * REG + d.nc) * d.A;
    const float x = to_f<T>(preds[g.n * per_img + (long)lane * d.A + a]);
    float p, lse, ev;
    side_softmax(x, bin, p, lse, ev);
    const float ax = to_f<T>(anchors[a]), ay = to_f<T>(anchors[d.A + a]), st = to_f<T>(strides[a]);
    const float px = ax * st, py = ay * st;
    // ---- DFL, weighted by t
    const float tv = side == 0 ? (px - g.x1) / st : side == 1 ? (py - g.y1) / st : side == 2 ? (g.x2 - px) / st : (g.y2 - py) / st;
    float contrib, gbody;
    dfl_pair(tv, bin, lse - x, p, contrib, gbody);
    const float dfl = sides_sum(contrib) * 0.25f;
    const float cd = d.lambda_dfl * t / tss * 0.25f;
    float gacc = cd * gbody;
    // ---- CIoU, weighted by t
    float dc[4];
    const float ciou = ciou_terms(w.pbox[slot], g, dc);
    const float cb = d.lambda_box * t / tss;
    const float gs = side == 0 ? st * (cb * dc[0]) : side == 1 ? st * (cb * dc[1]) : side == 2 ? -st * (cb * dc[2]) : -st * (cb * dc[3]);
    gacc += gs * p * ((float)bin - ev);
    if (dpreds) dpreds[g.n * per_img + (long)lane * d.A + a] = from_f<T>(gacc * gsc);
    if (lane == 0) w.ebox[j * KMAX + r] = t * (1.f - ciou), w.edfl[j * KMAX + r] = t * dfl;
}

template <typename T, int V>
__global__ __launch_bounds__(256) void k_tal_final(TalDims d, int nblk, int fblk, const T* __restrict__ preds, T* __restrict__ dpreds,
                                                   const T* __restrict__ anchors, const T* __restrict__ strides,
                                                   const float* __restrict__ gt, const int* __restrict__ gt_img,
                                                   const int* __restrict__ gt_off, const float* __restrict__ grad_scale, TalWs w) {
    const float gsc = grad_scale ? *grad_scale : 1.f;
    const int b = blockIdx.x;
    if (b < nblk) {
        float coef = d.lambda_cls / *w.tss;
        if (grad_scale) coef *= gsc;                          // applied in fp32, before the one rounding
        dense_part<T, V>(d, b, nblk, preds, dpreds, w, coef);
    } else if (b < nblk + fblk) {
        fill_part<T, V>(d, b - nblk, fblk, dpreds, w);
    } else {
        positive_part<T>(d, b - nblk - fblk, preds, dpreds, anchors, strides, gt, gt_img, gt_off, w, gsc);
    }
}

// one block: the class partials and the per-entry values, strided per thread in double, a fixed butterfly per wave, the four
// waves in order
__global__ __launch_bounds__(256) void k_tal_finish(TalDims d, int nblk, const int* __restrict__ gt_off, TalWs w, float* __restrict__ out) {
    __shared__ double red[3][4];
    const int entries = live_rows(gt_off, d.N, d.G) * KMAX;
    double cls = 0.0, box = 0.0, dfl = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) cls += w.partial[i];
    for (int i = threadIdx.x; i < entries; i += 256) box += (double)w.ebox[i], dfl += (double)w.edfl[i];
    cls = wave_sum_d(cls), box = wave_sum_d(box), dfl = wave_sum_d(dfl);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = cls, red[1][threadIdx.x >> 6] = box, red[2][threadIdx.x >> 6] = dfl;
    __syncthreads();
    if (threadIdx.x) return;
    const double tss = (double)*w.tss;
    cls = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / tss;
    box = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / tss;
    dfl = ((red[2][0] + red[2][1]) + (red[2][2] + red[2][3])) / tss;
    out[0] = (float)(d.lambda_box * box + d.lambda_cls * cls + d.lambda_dfl * dfl);
    out[1] = (float)box;
    out[2] = (float)cls;
    out[3] = (float)dfl;
}

}  // namespace

extern "C" {

// pbox, the owner word and the (label, t) word per (n, a); per GT row the list of KMAX (anchor, align, iou) entries, the two
// per-entry values, count, ma, mi and the sum of t; the class partials; tss.  No G x A array.
size_t yolo_loss_tal_workspace_bytes(int N, int A, int G) { return carve(nullptr, N, A, G).bytes; }

// Same buffers as yolo_loss_dfl_qfl (gt fp32 [G][5] grouped by image, gt_off int32 [N+1], gt_img int32 [G]; G = row capacity,
// live count gt_off[N] read on the device; dpreds may be null; grad_scale optional device scalar).  out: fp32[4] = {total,
// box, cls, dfl}.  1 <= topk <= 16.
int yolo_loss_tal(const void* preds, const void* anchors, const void* strides, int dtype, int N, int nc, int A,
                  const float* gt, const int* gt_off, const int* gt_img, int G, int topk, float alpha, float beta,
                  float lambda_box, float lambda_cls, float lambda_dfl, void* dpreds, float* out, void* workspace,
                  const float* grad_scale, hipStream_t st) {
    if (N < 1 || A < 1 || nc < 1 || G < 0 || topk < 1 || topk > KMAX) return YOLO_ERR_ARG;
    TalDims d{N, A, nc, G, topk, alpha, beta, lambda_box, lambda_cls, lambda_dfl};
    const TalWs w = carve(workspace, N, A, G);
    const long NA = (long)N * A;
    const int rows = ceil_div(G > 0 ? G : 1, 4);
    YOLO_DISPATCH_T(dtype, {
        constexpr int VV = vec_of<T>::N;
        const bool vec = (A % VV == 0) && ((uintptr_t)preds % 16 == 0) && (!dpreds || (uintptr_t)dpreds % 16 == 0);
        const int V = vec ? VV : 1;
        long it = (long)N * ((nc + CH - 1) / CH) * (A / V);
        int nblk = (int)((it + 255) / 256 < DENSE_BLOCKS ? (it + 255) / 256 : DENSE_BLOCKS);
        it = (long)N * (4 * REG / CH) * (A / V);
        int fblk = !dpreds ? 0 : (int)((it + 255) / 256 < FILL_BLOCKS ? (it + 255) / 256 : FILL_BLOCKS);
        const int grid = nblk + fblk + 4 * G;
        hipLaunchKernelGGL((k_tal_decode<T>), dim3(ceil_div(NA, 256)), dim3(256), 0, st, d, (const T*)preds, (const T*)anchors,
                           (const T*)strides, w);
        if (G > 0) hipLaunchKernelGGL((k_tal_topk<T>), dim3(G), dim3(256), 0, st, d, (const T*)preds, (const T*)anchors,
                                      (const T*)strides, gt, gt_img, gt_off, w);
        if (G > 0) hipLaunchKernelGGL(k_tal_resolve, dim3(rows), dim3(256), 0, st, d, gt, gt_img, gt_off, w);
        hipLaunchKernelGGL(k_tal_tss, dim3(1), dim3(256), 0, st, d, gt_off, w);
        if (vec) hipLaunchKernelGGL((k_tal_final<T, VV>), dim3(grid), dim3(256), 0, st, d, nblk, fblk, (const T*)preds, (T*)dpreds,
                                    (const T*)anchors, (const T*)strides, gt, gt_img, gt_off, grad_scale, w);
        else hipLaunchKernelGGL((k_tal_final<T, 1>), dim3(grid), dim3(256), 0, st, d, nblk, fblk, (const T*)preds, (T*)dpreds,
                                (const T*)anchors, (const T*)strides, gt, gt_img, gt_off, grad_scale, w);
        hipLaunchKernelGGL(k_tal_finish, dim3(1), dim3(256), 0, st, d, nblk, gt_off, w, out);
    });
    return YOLO_LAUNCH_CHECK();
}

}  // extern "C"
