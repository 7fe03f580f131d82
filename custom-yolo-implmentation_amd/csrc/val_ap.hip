// COCO average precision on the device: the matching of COCOeval.evaluateImg (no crowd, no ignore regions) at
// up to ten IoU thresholds, and COCOeval.accumulate's 101-point precision table for area "all".  It stands beside the
// reference's `"mAP"` (src/training/metrics.py:159-191), which is a precision at one threshold and one confidence cut.
//
//   k_ap_match : one wave per image walks yolo_nms's rows in the order given; per threshold a row takes the free GT of its
//                class with the largest IoU >= min(thr, 1 - 1e-10), the HIGHEST index among equal IoUs (COCOeval's scan
//                replaces on >=); ten independent `taken` sets; IoU in double from the fp32 values; a NaN IoU never matches.
//                Writes per row a sort key (class ascending, then score descending) and the bit set of thresholds matched.
//   k_ap_curve : one workgroup per (class, threshold) on the rows sorted by key: cumulative TP / FP, recall, precision with
//                eps = 2^-52, the envelope from the right and the lookup at the 101 recall thresholds, in one backward pass.
// Every compared quantity is an integer or a double formed in a fixed operation order: built with -ffp-contract=off.
#include "common.h"

namespace {

constexpr int AP_MAX_THR = 10;
constexpr int AP_SLOTS = 16;        // targets per lane: images with up to 1024 ground-truth boxes (as yolo_val_match)
constexpr int AP_NREC = 101;        // recall thresholds of the table

__device__ __forceinline__ unsigned score_ord(float s) {       // order-preserving map of an fp32 bit pattern to uint32
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(64) void k_ap_match(const float* __restrict__ det /*[N][K][6]*/, const int* __restrict__ count,
                                                 int K, const float* __restrict__ gt /*[total][5]*/,
                                                 const int* __restrict__ gt_off, const double* __restrict__ iou_thr, int n_thr,
                                                 int nc, long long* __restrict__ key /*[N][K]*/, unsigned* __restrict__ tp,
                                                 long long* __restrict__ gt_count, int* __restrict__ status) {
    const int img = blockIdx.x, lane = threadIdx.x;
    const float* P = det + (long)img * K * 6;
    long long* okey = key + (long)img * K;
    unsigned* otp = tp + (long)img * K;
    int n = count[img];
    n = n < 0 ? 0 : (n > K ? K : n);
    const int g0 = gt_off[img], m = gt_off[img + 1] - g0;
    const long long invalid = (long long)nc << 32;
    if (m > 64 * AP_SLOTS) {                                    // the image contributes nothing
        if (lane == 0) *status = 1;
        n = 0;
    }
    // keys of all K rows; tp of the rows that are ignored (the matching below writes the others)
    for (int i = lane; i < K; i += 64) {
        const long long c = (long long)P[(long)i * 6 + 5];
        const bool ok = i < n && c >= 0 && c < nc;
        okey[i] = ok ? ((c << 32) | (long long)(0xFFFFFFFFu - score_ord(P[(long)i * 6 + 4]))) : invalid;
        if (!ok) otp[i] = 0u;
    }
    if (m > 64 * AP_SLOTS) return;
    const float* G = gt + (long)g0 * 5;
    const int nslot = (m + 63) >> 6;
    // this lane's targets j = lane + 64 s: class, corners and area in double
    long long gc[AP_SLOTS];
    double gx1[AP_SLOTS], gy1[AP_SLOTS], gx2[AP_SLOTS], gy2[AP_SLOTS], ga[AP_SLOTS];
#pragma unroll
    for (int s = 0; s < AP_SLOTS; ++s) {
        const int j = lane + 64 * s;
        gc[s] = -1;
        gx1[s] = gy1[s] = gx2[s] = gy2[s] = ga[s] = 0.0;
        if (j < m) {
            const double cx = G[j * 5], cy = G[j * 5 + 1], hw = (double)G[j * 5 + 2] / 2.0, hh = (double)G[j * 5 + 3] / 2.0;
            const long long c = (long long)G[j * 5 + 4];
            gx1[s] = cx - hw; gy1[s] = cy - hh; gx2[s] = cx + hw; gy2[s] = cy + hh;
            ga[s] = (gx2[s] - gx1[s]) * (gy2[s] - gy1[s]);
            if (c >= 0 && c < nc) {
                gc[s] = c;
                atomicAdd(reinterpret_cast<unsigned long long*>(gt_count + c), 1ull);
            }
        }
    }
    __shared__ double thr[AP_MAX_THR];
    if (lane < n_thr) {
        const double v = iou_thr[lane], cap = 1.0 - 1e-10;
        thr[lane] = v < cap ? v : cap;
    }
    __syncthreads();
    double thr_lo = INFINITY;
    for (int t = 0; t < n_thr; ++t) thr_lo = thr[t] < thr_lo ? thr[t] : thr_lo;
    unsigned taken[AP_SLOTS];                                   // bit t of taken[s]: target lane + 64 s is matched at threshold t
#pragma unroll
    for (int s = 0; s < AP_SLOTS; ++s) taken[s] = 0u;

    for (int i = 0; i < n; ++i) {
        const long long pc = (long long)P[(long)i * 6 + 5];
        if (pc < 0 || pc >= nc) continue;                       // wave-uniform
        const double x1 = P[(long)i * 6], y1 = P[(long)i * 6 + 1], x2 = P[(long)i * 6 + 2], y2 = P[(long)i * 6 + 3];
        const double a1 = (x2 - x1) * (y2 - y1);
        double v[AP_SLOTS];
        bool any = false;
#pragma unroll
        for (int s = 0; s < AP_SLOTS; ++s) {
            v[s] = NAN;                                         // other class / no target: compares false with every threshold
            if (s < nslot && gc[s] == pc) {
                double iw = (x2 < gx2[s] ? x2 : gx2[s]) - (x1 > gx1[s] ? x1 : gx1[s]);
                double ih = (y2 < gy2[s] ? y2 : gy2[s]) - (y1 > gy1[s] ? y1 : gy1[s]);
                iw = iw > 0.0 ? iw : 0.0;
                ih = ih > 0.0 ? ih : 0.0;
                const double inter = iw * ih;
                const double iou = inter / ((a1 + ga[s]) - inter);
                v[s] = iou;                                     // a NaN compares false: never matches
                any |= iou >= thr_lo;
            }
        }
        unsigned bits = 0u;
        if (__ballot(any) != 0ull) {
            for (int t = 0; t < n_thr; ++t) {
                const double thr_t = thr[t];
                double best = -1.0;
                int bj = -1;
#pragma unroll
                for (int s = 0; s < AP_SLOTS; ++s)              // ascending index inside the lane: >= keeps the highest
                    if (!((taken[s] >> t) & 1u) && v[s] >= thr_t && v[s] >= best) { best = v[s]; bj = lane + 64 * s; }
                if (__ballot(bj >= 0) == 0ull) continue;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {              // largest IoU, highest target index on ties
                    const double ob = __shfl_xor(best, o, 64);
                    const int oj = __shfl_xor(bj, o, 64);
                    if (ob > best || (ob == best && oj > bj)) { best = ob; bj = oj; }
                }
                bits |= 1u << t;
                if ((bj & 63) == lane) {
                    const int sj = bj >> 6;
#pragma unroll
                    for (int s = 0; s < AP_SLOTS; ++s)
                        if (s == sj) taken[s] |= 1u << t;
                }
            }
        }
        if (lane == 0) otp[i] = bits;
    }
}

// inclusive prefix sum (forward) of one int per thread over the 256 threads; total of the block in `total`
__device__ __forceinline__ int block_incl_sum(int v, int* lds4, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) lds4[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; ++w) inc += lds4[w];
    total = lds4[0] + lds4[1] + lds4[2] + lds4[3];
    return inc;
}

// inclusive suffix maximum (from the right) of one double per thread over the 256 threads; maximum of the block in `all`
__device__ __forceinline__ double block_suffix_max(double v, double* lds4, double& all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mx = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_down(mx, o, 64);
        if (lane + o < 64 && t > mx) mx = t;
    }
    __syncthreads();
    if (lane == 0) lds4[wave] = mx;
    __syncthreads();
    for (int w = wave + 1; w < 4; ++w) mx = lds4[w] > mx ? lds4[w] : mx;
    all = lds4[0];
    for (int w = 1; w < 4; ++w) all = lds4[w] > all ? lds4[w] : all;
    return mx;
}

__device__ __forceinline__ int lower_bound_key(const long long* __restrict__ key, int D, long long want) {
    int lo = 0, hi = D;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_ap_curve(const long long* __restrict__ key, const unsigned* __restrict__ tp, int D,
                                                  const long long* __restrict__ gt_count,
                                                  const double* __restrict__ rec_thr /*[101]*/,
                                                  double* __restrict__ precision /*[nc][n_thr][101]*/) {
    __shared__ double tab[AP_NREC], rthr[AP_NREC], mx4[4];
    __shared__ int sum4[4];
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    double* out = precision + ((long)c * gridDim.y + t) * AP_NREC;
    const long long npig = gt_count[c];
    if (npig == 0) {                                            // class absent: excluded from the means
        if (tid < AP_NREC) out[tid] = -1.0;
        return;
    }
    if (tid < AP_NREC) { tab[tid] = 0.0; rthr[tid] = rec_thr[tid]; }
    const int lo = lower_bound_key(key, D, (long long)c << 32), hi = lower_bound_key(key, D, (long long)(c + 1) << 32);
    const int L = hi - lo, nchunk = (L + 255) >> 8;
    int part = 0;
    for (int i = tid; i < L; i += 256) part += (int)((tp[lo + i] >> t) & 1u);
    int tp_total;
    block_incl_sum(part, sum4, tp_total);                       // (its barriers also publish tab / rthr)
    const double dn = (double)npig, eps = 2.220446049250313e-16;   // np.spacing(1) = 2^-52
    int after = 0;                                              // TP in the chunks behind this one
    double carry = -INFINITY;                                   // envelope of the chunks behind this one
    for (int b = nchunk - 1; b >= 0; --b) {
        const int i = b * 256 + tid;                            // index inside the segment
        const int bit = i < L ? (int)((tp[lo + i] >> t) & 1u) : 0;
        int chunk_tp;
        const int inc = block_incl_sum(bit, sum4, chunk_tp);
        const int tpi = tp_total - after - chunk_tp + inc;      // inclusive TP count of row i
        const double dtp = (double)tpi, dfp = (double)(i + 1) - dtp;
        const double pr = i < L ? dtp / (dfp + dtp + eps) : -INFINITY;
        double chunk_max;
        double env = block_suffix_max(pr, mx4, chunk_max);
        env = carry > env ? carry : env;
        if (i < L && (bit || i == 0)) {
            const double rc = dtp / dn, prev = i == 0 ? -INFINITY : (double)(tpi - bit) / dn;
            for (int k = 0; k < AP_NREC; ++k)
                if (rthr[k] > prev && rthr[k] <= rc) tab[k] = env;
        }
        after += chunk_tp;
        carry = chunk_max > carry ? chunk_max : carry;
    }
    __syncthreads();
    if (tid < AP_NREC) out[tid] = tab[tid];
}

}  // namespace

extern "C" {

// det: yolo_nms's rows fp32 [N][K][6] (x1, y1, x2, y2, score, cls; descending score) with count int32 [N]; gt fp32 [total][5]
// (cx, cy, w, h, cls), image i owning rows gt_off[i] .. gt_off[i+1]; iou_thr: n_thr doubles ON THE DEVICE, 1 <= n_thr <= 10.
// key int64 [N][K] = (cls << 32) | (0xFFFFFFFF - ord(score)), nc << 32 for rows at or past count and rows of a class outside
// [0, nc); tp uint32 [N][K], bit t = matched at threshold t; gt_count int64 [nc], accumulated; status int32 [1], set to 1 by
// an image with more than 1024 targets (it contributes nothing).
int yolo_ap_match(const float* det, const int* count, int N, int K, const float* gt, const int* gt_off, const double* iou_thr,
                  int n_thr, int nc, long long* key, unsigned* tp, long long* gt_count, int* status, hipStream_t st) {
    if (N < 1 || K < 1 || nc < 1 || n_thr < 1 || n_thr > AP_MAX_THR) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_ap_match, dim3(N), dim3(64), 0, st, det, count, K, gt, gt_off, iou_thr, n_thr, nc, key, tp, gt_count,
                       status);
    return YOLO_LAUNCH_CHECK();
}

// key / tp: the D rows of every yolo_ap_match call, sorted ascending by key with a STABLE sort; rec_thr: the 101 recall
// thresholds (np.linspace(0, 1, 101)) on the device; precision: double [nc][n_thr][101], -1 for a class without targets.
int yolo_ap_curve(const long long* key, const unsigned* tp, long D, const long long* gt_count, const double* rec_thr, int nc,
                  int n_thr, double* precision, hipStream_t st) {
    if (D < 0 || D >= (1L << 31) || nc < 1 || nc > 65535 || n_thr < 1 || n_thr > AP_MAX_THR) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_ap_curve, dim3(nc, n_thr), dim3(256), 0, st, key, tp, (int)D, gt_count, rec_thr, precision);
    return YOLO_LAUNCH_CHECK();
}

}  // extern "C"
