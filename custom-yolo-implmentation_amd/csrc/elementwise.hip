// HBM-bound NHWC kernels: layout changes, channel copies, BatchNorm (+SiLU, +residual) forward and
// backward, SPPF max-pool, nearest x2 upsample.  One 16-byte packet per lane wherever the channel
// count allows it (guide: Guideline 13), fp32 arithmetic, fp32 statistics.
#include "common.h"
#include "bn_coef.h"

namespace {

constexpr int TPB = 256;
constexpr int RS_ROWS = 2;        // pixel rows (independent 16-byte loads per tensor) in flight per thread
constexpr int RS_MAXBLK = 256 * 8;  // row-strided grids: at most 8 workgroups per CU

template <typename T> __host__ bool vec_ok(const void* p, long ld, int C) {
    constexpr int V = vec_of<T>::N;
    return (C % V == 0) && (ld % V == 0) && ((reinterpret_cast<uintptr_t>(p) % 16) == 0);
}

// ---------------------------------------------------------------------------------------------
// (n, c, m) <-> NHWC tiled transposes.  "ncm" side: elem(n,c,p) at base[n*sn + c*sc + off + p].
// ---------------------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ void k_ncm_to_nhwc(const TI* __restrict__ src, long sn, long sc, long off,
                              TO* __restrict__ dst, int ld, int C, int HW) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 8 rows of 32
    for (int r = ty; r < 32; r += 8) {
        int c = c0 + r, p = p0 + tx;
        tile[r][tx] = (c < C && p < HW) ? to_f<TI>(src[n * sn + c * sc + off + p]) : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        int p = p0 + r, c = c0 + tx;
        if (p < HW && c < C) dst[((long)n * HW + p) * ld + c] = from_f<TO>(tile[tx][r]);
    }
}

template <typename TI, typename TO>
__global__ void k_nhwc_to_ncm(const TI* __restrict__ src, int ld, TO* __restrict__ dst, long sn,
                              long sc, long off, int C, int HW) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        int p = p0 + r, c = c0 + tx;
        tile[r][tx] = (p < HW && c < C) ? to_f<TI>(src[((long)n * HW + p) * ld + c]) : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        int c = c0 + r, p = p0 + tx;
        if (c < C && p < HW) dst[n * sn + c * sc + off + p] = from_f<TO>(tile[tx][r]);
    }
}

// The head's six branch outputs <-> the (N, no, M) prediction tensor in ONE launch each way (HeadPack): a problem table in
// the kernel arguments, a workgroup finds its branch from the prefix of tile counts and transposes one 32 x 32 tile.
constexpr int HEAD_GROUP = 8;
struct HeadGroup {
    void* t[HEAD_GROUP];            // NHWC branch tensors
    int ld[HEAD_GROUP], C[HEAD_GROUP], HW[HEAD_GROUP], c_off[HEAD_GROUP], m_off[HEAD_GROUP], tp[HEAD_GROUP];   // tp: pixel tiles
    int start[HEAD_GROUP + 1];      // first workgroup (per image) of branch i
    int n;
};

template <typename T, bool PACK>
__global__ __launch_bounds__(256) void k_head_group(HeadGroup g, T* __restrict__ preds, long sn, long sc) {
    __shared__ float tile[32][33];
    int bi = 0;
#pragma unroll
    for (int i = 1; i < HEAD_GROUP; ++i)
        if (i < g.n && (int)blockIdx.x >= g.start[i]) bi = i;
    T* x; int ld, C, HW, c_off, m_off, tp, st;
#define HG_PICK(I) case I: x = (T*)g.t[I]; ld = g.ld[I]; C = g.C[I]; HW = g.HW[I]; c_off = g.c_off[I]; m_off = g.m_off[I]; tp = g.tp[I]; st = g.start[I]; break;
    switch (bi) {
        HG_PICK(1) HG_PICK(2) HG_PICK(3) HG_PICK(4) HG_PICK(5) HG_PICK(6) HG_PICK(7)
        default: x = (T*)g.t[0]; ld = g.ld[0]; C = g.C[0]; HW = g.HW[0]; c_off = g.c_off[0]; m_off = g.m_off[0]; tp = g.tp[0]; st = g.start[0]; break;
    }
#undef HG_PICK
    const int tl = (int)blockIdx.x - st;
    const int n = blockIdx.y, p0 = (tl % tp) * 32, c0 = (tl / tp) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    T* pr = preds + n * sn + (long)c_off * sc + m_off;
    if (PACK) {
        for (int r = ty; r < 32; r += 8) {
            const int p = p0 + r, c = c0 + tx;
            tile[r][tx] = (p < HW && c < C) ? to_f<T>(x[((long)n * HW + p) * ld + c]) : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int c = c0 + r, p = p0 + tx;
            if (c < C && p < HW) pr[c * sc + p] = from_f<T>(tile[tx][r]);
        }
    } else {
        for (int r = ty; r < 32; r += 8) {
            const int c = c0 + r, p = p0 + tx;
            tile[r][tx] = (c < C && p < HW) ? to_f<T>(pr[c * sc + p]) : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int p = p0 + r, c = c0 + tx;
            if (p < HW && c < C) x[((long)n * HW + p) * ld + c] = from_f<T>(tile[tx][r]);
        }
    }
}

// The same with 16-byte accesses on both sides (16-bit tensors, C % 8 == 0, HW / M / offsets multiples of 8): a workgroup
// owns 64 pixels x all C channels of one branch and image; the tile crosses LDS as [pixel][channel] (row stride C + 2
// elements: the 8 strided 2-byte reads / writes of a transposing thread fall in different banks).
template <typename T, bool PACK>
__global__ __launch_bounds__(256) void k_head_group_vec(HeadGroup g, T* __restrict__ preds, long sn, long sc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hg_raw[];
    T* tile = reinterpret_cast<T*>(hg_raw);                   // [64][C + 2]
    int bi = 0;
#pragma unroll
    for (int i = 1; i < HEAD_GROUP; ++i)
        if (i < g.n && (int)blockIdx.x >= g.start[i]) bi = i;
    T* x; int ld, C, HW, c_off, m_off, st;
#define HG_PICK(I) case I: x = (T*)g.t[I]; ld = g.ld[I]; C = g.C[I]; HW = g.HW[I]; c_off = g.c_off[I]; m_off = g.m_off[I]; st = g.start[I]; break;
    switch (bi) {
        HG_PICK(1) HG_PICK(2) HG_PICK(3) HG_PICK(4) HG_PICK(5) HG_PICK(6) HG_PICK(7)
        default: x = (T*)g.t[0]; ld = g.ld[0]; C = g.C[0]; HW = g.HW[0]; c_off = g.c_off[0]; m_off = g.m_off[0]; st = g.start[0]; break;
    }
#undef HG_PICK
    const int n = blockIdx.y, p0 = ((int)blockIdx.x - st) * 64;
    const int LDT = C + 2, cpr = C / 8;                       // 16-byte chunks per pixel row
    T* pr = preds + n * sn + (long)c_off * sc + m_off;
    T* xr = x + ((long)n * HW + p0) * ld;
    const int npx = HW - p0 < 64 ? HW - p0 : 64;              // multiple of 8
    if (PACK) {
        for (int i = threadIdx.x; i < npx * cpr; i += 256) {
            const int p = i / cpr, ch = (i - p * cpr) * 8;
            const pack_t<T, 8> v = load_raw<T, 8>(xr + (long)p * ld + ch);
#pragma unroll
            for (int e = 0; e < 8; ++e) tile[p * LDT + ch + e] = v.v[e];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < C * (npx / 8); i += 256) {
            const int c = i / (npx / 8), pg = (i - c * (npx / 8)) * 8;
            pack_t<T, 8> v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v.v[e] = tile[(pg + e) * LDT + c];
            *reinterpret_cast<pack_t<T, 8>*>(pr + c * sc + p0 + pg) = v;
        }
    } else {
        for (int i = threadIdx.x; i < C * (npx / 8); i += 256) {
            const int c = i / (npx / 8), pg = (i - c * (npx / 8)) * 8;
            const pack_t<T, 8> v = load_raw<T, 8>(pr + c * sc + p0 + pg);
#pragma unroll
            for (int e = 0; e < 8; ++e) tile[(pg + e) * LDT + c] = v.v[e];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < npx * cpr; i += 256) {
            const int p = i / cpr, ch = (i - p * cpr) * 8;
            pack_t<T, 8> v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v.v[e] = tile[p * LDT + ch + e];
            *reinterpret_cast<pack_t<T, 8>*>(xr + (long)p * ld + ch) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// channel-slice copy / accumulate (concat, chunk backward, gradient fan-in)
// ---------------------------------------------------------------------------------------------
template <typename T, int V, bool ACC>
__global__ void k_copy_channels(const T* __restrict__ src, int lds_, T* __restrict__ dst, int ldd,
                                long npix, int cv) {
    long total = npix * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long p = i / cv;
        int cg = (int)(i - p * cv);
        float a[V];
        load_pack<T, V>(src + p * lds_ + cg * V, a);
        if (ACC) {
            float b[V];
            load_pack<T, V>(dst + p * ldd + cg * V, b);
#pragma unroll
            for (int j = 0; j < V; ++j) a[j] += b[j];
        }
        store_pack<T, V>(dst + p * ldd + cg * V, a);
    }
}

// dst = sum of up to four channel-slice tensors (fp32 accumulate, one rounding): the gradient of a tensor with several
// consumers in ONE pass (autograd's own accumulation is one ATen add -- three passes over memory -- per extra consumer)
struct AddSrcs { const void* p[4]; int ld[4]; };
template <typename T, int V, int NS>
__global__ void k_add_n(AddSrcs s, T* __restrict__ dst, int ldd, long npix, int cv) {
    long total = npix * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long p = i / cv;
        int cg = (int)(i - p * cv);
        float a[V];
        load_pack<T, V>((const T*)s.p[0] + p * s.ld[0] + cg * V, a);
#pragma unroll
        for (int k = 1; k < NS; ++k) {
            float b[V];
            load_pack<T, V>((const T*)s.p[k] + p * s.ld[k] + cg * V, b);
#pragma unroll
            for (int j = 0; j < V; ++j) a[j] += b[j];
        }
        store_pack<T, V>(dst + p * ldd + cg * V, a);
    }
}

// ---------------------------------------------------------------------------------------------
// BatchNorm (+SiLU, +residual): per-channel reductions over pixels, finalizes, normalise / gradient passes.
// The six kernels that touch every element share one row-strided pixel walk (rs_walk).
// ---------------------------------------------------------------------------------------------
// (sigmoid_rcp and act_grad: bn_coef.h, shared with the stem's one-pass backward)
__device__ __forceinline__ float act_fwd(float z, int act) { return act == 0 ? z : z * sigmoid_rcp(z); }

// Row-strided walk: a workgroup is rpb = TPB / tpr pixel rows of tpr lanes; a thread keeps ONE channel group (cg: V
// channels, whose constants live in registers or LDS; cl: the group's index within the workgroup) and walks pixel rows
// r, r + rpb, ... of its workgroup's share: no per-element index division.  blockIdx.y covers channel groups beyond tpr.
// Threads past the last whole row of the workgroup or past the last channel group are not active.
struct RsThread { int rpb, r, cl, cg; bool active; };
__device__ __forceinline__ RsThread rs_thread(int tpr, int cv) {
    RsThread t;
    t.rpb = TPB / tpr;
    t.r = threadIdx.x / tpr;
    t.cl = threadIdx.x - t.r * tpr;
    t.cg = blockIdx.y * tpr + t.cl;
    t.active = (t.r < t.rpb) && (t.cg < cv);
    return t;
}

// one(p, packet of a, packet of b) for every pixel p of active thread t; without has_b the second tensor is not read.
// The main loop keeps RS_ROWS independent 16-byte loads per tensor in flight and has no bounds tests; the tail takes
// one row at a time.  (Start row and step are formed here, after the caller's early exit, not in rs_thread.)
// The tail runs fewer than RS_ROWS times per thread: left to itself the compiler vectorizes it four wide in the
// one-element-per-lane backward apply (68 registers instead of 40, a wave less per SIMD), for nothing.
template <typename T, int V, typename F>
__device__ __forceinline__ void rs_walk(const RsThread& t, const T* __restrict__ a, int lda, const T* __restrict__ b, int ldb, bool has_b,
                                        long npix, F one) {
    const long step = (long)gridDim.x * t.rpb;
    long p = (long)blockIdx.x * t.rpb + t.r;
    for (; p + (RS_ROWS - 1) * step < npix; p += RS_ROWS * step) {
        pack_t<T, V> ra[RS_ROWS], rb[RS_ROWS];
#pragma unroll
        for (int k = 0; k < RS_ROWS; ++k) {
            ra[k] = load_raw<T, V>(a + (p + k * step) * lda + t.cg * V);
            if (has_b) rb[k] = load_raw<T, V>(b + (p + k * step) * ldb + t.cg * V);
        }
#pragma unroll
        for (int k = 0; k < RS_ROWS; ++k) one(p + k * step, ra[k], rb[k]);
    }
#pragma clang loop vectorize(disable)
    for (; p < npix; p += step) {
        pack_t<T, V> pa = load_raw<T, V>(a + p * lda + t.cg * V), pb;
        if (has_b) pb = load_raw<T, V>(b + p * ldb + t.cg * V);
        one(p, pa, pb);
    }
}

// Per-channel sums of one workgroup's pixels, handed to sink(index into a [2][C] row, value):
//   MODE 0: (sum y, sum y^2)                      -- BN batch statistics / bias gradient
//   MODE 1: (sum dz, sum dz*y), dz = dout*act'(z), z = y*scale+shift   (raw; the finalize / apply kernel centres the
//           second sum into sum(dz*yhat) in double)
// The activation is a template parameter: no per-element select between SiLU and identity.
template <typename T, int V, int MODE, int ACT, typename Sink>
__device__ __forceinline__ void channel_sums(const T* __restrict__ y, int ldy, const T* __restrict__ dout, int ldd,
                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                             long npix, int C, int tpr, Sink sink) {
    __shared__ float red[TPB][2 * V + 1];
    const int cv = C / V;
    const RsThread th = rs_thread(tpr, cv);
    float s[V], q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = q[j] = 0.f;
    if (th.active) {
        float sc[V], sh[V];
        if (MODE == 1) {
#pragma unroll
            for (int j = 0; j < V; ++j) { sc[j] = scale[th.cg * V + j]; sh[j] = shift[th.cg * V + j]; }
        }
        rs_walk<T, V>(th, y, ldy, dout, ldd, MODE == 1, npix, [&](long, const pack_t<T, V>& pa, const pack_t<T, V>& pd) {
            float a[V], d[V];
            unpack<T, V>(pa, a);
            if (MODE == 1) unpack<T, V>(pd, d);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (MODE == 0) { s[j] += a[j]; q[j] += a[j] * a[j]; }
                else {
                    float dz = d[j] * act_grad(a[j] * sc[j] + sh[j], ACT);
                    s[j] += dz;
                    q[j] += dz * a[j];
                }
            }
        });
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { red[threadIdx.x][j] = s[j]; red[threadIdx.x][V + j] = q[j]; }
    __syncthreads();
    // one thread per (channel group, value): tpr*2V outputs, each the sum over the workgroup's rpb pixel rows
    // (a single row of threads walking all rows serially cost 10-20 us per workgroup on narrow layers)
    for (int t = threadIdx.x; t < tpr * 2 * V; t += TPB) {
        const int cl = t / (2 * V), j = t - cl * 2 * V;
        float a = 0.f;
#pragma unroll 8
        for (int rr = 0; rr < th.rpb; ++rr) a += red[rr * tpr + cl][j];
        const int cgo = blockIdx.y * tpr + cl;
        if (cgo < cv) sink((j / V) * C + cgo * V + (j % V), a);
    }
}

// deterministic path: workgroup x stores its sums to its own row of partial[gridDim.x][2][C]; a finalize kernel adds the rows
template <typename T, int V, int MODE, int ACT>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(5, 8)))
void k_channel_reduce(const T* __restrict__ y, int ldy, const T* __restrict__ dout, int ldd, const float* __restrict__ scale,
                      const float* __restrict__ shift, long npix, int C, float* __restrict__ partial, int tpr) {
    float* o = partial + (long)blockIdx.x * 2 * C;
    channel_sums<T, V, MODE, ACT>(y, ldy, dout, ldd, scale, shift, npix, C, tpr, [&](int i, float a) { o[i] = a; });
}

// ---------------------------------------------------------------------------------------------
// Training-mode BN without finalize launches.  Per-channel sums live in a caller-zeroed accumulator
// acc[BN_REPL][2][C] (fp32): producers (the conv epilogue, or k_channel_acc below) add their partial
// sums into replica (workgroup index mod BN_REPL) with float atomics -- spreading a layer's adds over
// 8 rows per channel keeps the global-atomic unit out of its contended regime -- and every consumer
// workgroup folds the replicas and derives the per-channel constants for its own channel group in
// its prologue.  Workgroup (0, y) also publishes mean / invstd / running statistics (forward) or
// dgamma / dbeta (backward).
// ---------------------------------------------------------------------------------------------
// BatchNorm parameters and buffers travel in their own element type: PIn / PIo of bn_coef.h.
constexpr int BN_REPL = 8;

// per-channel constants of a workgroup's cw = tpr*V channels (dynamic LDS): [2][cw] scale, shift in the forward kernel,
// [5][cw] scale, shift, A, B, D in the backward apply kernels
extern __shared__ float cf[];

// channel c's two sums over the replicas, in double
__device__ __forceinline__ void acc_fold(const float* __restrict__ acc, int C, int c, double& s, double& q) {
    s = 0.0; q = 0.0;
#pragma unroll
    for (int r = 0; r < BN_REPL; ++r) { s += acc[(long)r * 2 * C + c]; q += acc[(long)r * 2 * C + C + c]; }
}

// default path: the same sums, added into replica (workgroup index mod BN_REPL) of acc.  scale / shift of MODE 1 are the
// forward's.
template <typename T, int V, int MODE, int ACT>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(5, 8)))
void k_channel_acc(const T* __restrict__ y, int ldy, const T* __restrict__ dout, int ldd, const float* __restrict__ scale,
                   const float* __restrict__ shift, long npix, int C, float* __restrict__ acc, int tpr) {
    float* o = acc + (long)(blockIdx.x % BN_REPL) * 2 * C;
    channel_sums<T, V, MODE, ACT>(y, ldy, dout, ldd, scale, shift, npix, C, tpr, [&](int i, float a) { atomicAdd(o + i, a); });
}

// Statistics -> coefficients of one channel, the only place this arithmetic is written.  Training-mode forward: (sum y,
// sum y^2) in double -> batch mean / biased variance (clamped at 0) -> invstd, scale, shift, and the unbiased variance the
// running statistics take (torch.nn.BatchNorm2d semantics).
struct BnFwdCoef { float mean, invstd, scale, shift, unbiased; };
__device__ __forceinline__ BnFwdCoef bn_fwd_coef(double s, double q, float count, float eps, float gamma, float beta) {
    const double m = s / count;
    double var = q / count - m * m;
    if (var < 0.0) var = 0.0;
    BnFwdCoef k;
    k.invstd = (float)(1.0 / sqrt(var + (double)eps));
    k.mean = (float)m;
    k.scale = gamma * k.invstd;
    k.shift = beta - (float)m * k.scale;
    k.unbiased = (float)(count > 1.f ? var * (count / (count - 1.0)) : var);
    return k;
}
// ... and their publication: the four saved vectors, the running statistics updated with momentum
__device__ __forceinline__ void bn_fwd_publish(const BnFwdCoef& k, int c, float momentum, float* __restrict__ mean,
                                               float* __restrict__ invstd, float* __restrict__ scale,
                                               float* __restrict__ shift, const PIo& rmean, const PIo& rvar) {
    mean[c] = k.mean;
    invstd[c] = k.invstd;
    scale[c] = k.scale;
    shift[c] = k.shift;
    if (rmean.p) {
        rmean.st(c, (1.f - momentum) * rmean.ld(c) + momentum * k.mean);
        rvar.st(c, (1.f - momentum) * rvar.ld(c) + momentum * k.unbiased);
    }
}
// Backward: (sum dz, sum dz*y) in double -> dbeta, dgamma and the three constants of dy = A*dz + B*y + D: bn_bwd_coef of
// bn_coef.h.

// acc[8][2][C] -> mean, invstd, scale, shift (+ running statistics): one thread per channel, 16 loads
__global__ void k_bn_finalize_acc(const float* __restrict__ acc, float count, int C, const void* __restrict__ gamma_,
                                  const void* __restrict__ beta_, void* __restrict__ rmean_, void* __restrict__ rvar_,
                                  float momentum, float eps, float* __restrict__ mean, float* __restrict__ invstd,
                                  float* __restrict__ scale, float* __restrict__ shift, int pdt, int bdt) {
    const PIn gamma{gamma_, pdt}; const PIn beta{beta_, pdt}; const PIo rmean{rmean_, bdt}, rvar{rvar_, bdt};
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s, q;
    acc_fold(acc, C, c, s, q);
    bn_fwd_publish(bn_fwd_coef(s, q, count, eps, gamma.ld(c), beta.ld(c)), c, momentum, mean, invstd, scale, shift, rmean, rvar);
}

// out = act(y*scale + shift) (+ res) over the pixels of thread th, scale / shift of its channels in registers
template <typename T, int V>
__device__ __forceinline__ void bn_act_fwd_rows(const RsThread& th, const T* __restrict__ y, int ldy, const T* __restrict__ res,
                                                int ldr, T* __restrict__ out, int ldo, long npix, const float (&sc)[V],
                                                const float (&sh)[V], int act) {
    const bool has_res = res;
    rs_walk<T, V>(th, y, ldy, res, ldr, has_res, npix, [&](long p, const pack_t<T, V>& pa, const pack_t<T, V>& pt) {
        float a[V], t[V];
        unpack<T, V>(pa, a);
        if (has_res) unpack<T, V>(pt, t);
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = act_fwd(a[j] * sc[j] + sh[j], act) + (has_res ? t[j] : 0.f);
        store_pack<T, V>(out + p * ldo + th.cg * V, a);
    });
}

// dy = A*dz + B*y + D, dz = dout*act'(y*scale + shift), over the pixels of thread th.  The five per-channel constants of
// the workgroup's channels sit in LDS (cf: [5][cw]) and are read at use: forty live coefficient registers per thread
// would halve the occupancy of a pure streaming kernel.
template <typename T, int V>
__device__ __forceinline__ void bn_act_bwd_rows(const RsThread& th, const T* __restrict__ dout, int ldd, const T* __restrict__ y,
                                                int ldy, T* __restrict__ dy, int lddy, long npix, int cw, int act) {
    const float* my = cf + th.cl * V;
    rs_walk<T, V>(th, y, ldy, dout, ldd, true, npix, [&](long p, const pack_t<T, V>& pa, const pack_t<T, V>& pd) {
        float a[V], d[V];
        unpack<T, V>(pa, a);
        unpack<T, V>(pd, d);
#pragma unroll
        for (int j = 0; j < V; ++j)
            d[j] = my[2 * cw + j] * (d[j] * act_grad(a[j] * my[j] + my[cw + j], act)) + my[3 * cw + j] * a[j] + my[4 * cw + j];
        store_pack<T, V>(dy + p * lddy + th.cg * V, d);
    });
}

// out = act(BN_batch(y)) (+ res) with the finalize folded in: every workgroup derives scale / shift of ITS channels
// from the statistics accumulator acc[8][2][C] (coalesced loads spread over the workgroup, then LDS); workgroup row 0
// also publishes mean / invstd / scale / shift and updates the running statistics.
template <typename T, int V, int ACT>
__global__ __launch_bounds__(TPB) void k_bn_act_fwd_train(const T* __restrict__ y, int ldy, const float* __restrict__ acc, float count,
                        const void* __restrict__ gamma_, const void* __restrict__ beta_, void* __restrict__ rmean_,
                        void* __restrict__ rvar_, float momentum, float eps, float* __restrict__ mean_out,
                        float* __restrict__ invstd_out, float* __restrict__ scale_out, float* __restrict__ shift_out,
                        const T* __restrict__ res, int ldr, T* __restrict__ out, int ldo, long npix, int C, int tpr, int pdt, int bdt) {
    const PIn gamma{gamma_, pdt}; const PIn beta{beta_, pdt}; const PIo rmean{rmean_, bdt}, rvar{rvar_, bdt};
    const int cw = tpr * V;
    for (int t = threadIdx.x; t < cw; t += TPB) {
        const int c = blockIdx.y * cw + t;
        float g = 0.f, sh0 = 0.f;
        if (c < C) {
            double s, q;
            acc_fold(acc, C, c, s, q);
            const BnFwdCoef k = bn_fwd_coef(s, q, count, eps, gamma.ld(c), beta.ld(c));
            g = k.scale;
            sh0 = k.shift;
            if (blockIdx.x == 0) bn_fwd_publish(k, c, momentum, mean_out, invstd_out, scale_out, shift_out, rmean, rvar);
        }
        cf[t] = g;
        cf[cw + t] = sh0;
    }
    __syncthreads();
    const RsThread th = rs_thread(tpr, C / V);
    if (!th.active) return;
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { sc[j] = cf[th.cl * V + j]; sh[j] = cf[cw + th.cl * V + j]; }
    bn_act_fwd_rows<T, V>(th, y, ldy, res, ldr, out, ldo, npix, sc, sh, ACT);
}

// dy = A*dz + B*y + D with the backward finalize folded in: acc[8][2][C] holds (sum dz, sum dz*y) of the reduction
// kernel (float atomics into 8 replicas); every workgroup folds the replicas of ITS channels and derives the five
// constants into LDS; workgroup row 0 also writes dgamma / dbeta.
template <typename T, int V, int ACT>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(5, 8)))
void k_bn_act_bwd_apply_train(const T* __restrict__ dout, int ldd, const T* __restrict__ y, int ldy,
                              const float* __restrict__ scale, const float* __restrict__ shift,
                              const void* __restrict__ gamma_, const float* __restrict__ mean,
                              const float* __restrict__ invstd, const float* __restrict__ acc, float count,
                              void* __restrict__ dgamma_, void* __restrict__ dbeta_, T* __restrict__ dy, int lddy,
                              long npix, int C, int tpr, int pdt) {
    const PIn gamma{gamma_, pdt}; const PIo dgamma{dgamma_, pdt}, dbeta{dbeta_, pdt};
    const int cw = tpr * V;
    for (int t = threadIdx.x; t < cw; t += TPB) {
        const int c = blockIdx.y * cw + t;
        float v0 = 0.f, v1 = 0.f;
        BnBwdCoef k{0.f, 0.f, 0.f, 0.f, 0.f};
        if (c < C) {
            double s, q;
            acc_fold(acc, C, c, s, q);
            k = bn_bwd_coef(s, q, count, gamma, mean, invstd, c);
            v0 = scale[c]; v1 = shift[c];
            if (blockIdx.x == 0) { dbeta.st(c, k.dbeta); dgamma.st(c, k.dgamma); }
        }
        cf[t] = v0; cf[cw + t] = v1; cf[2 * cw + t] = k.A; cf[3 * cw + t] = k.B; cf[4 * cw + t] = k.D;
    }
    __syncthreads();
    const RsThread th = rs_thread(tpr, C / V);
    if (!th.active) return;
    bn_act_bwd_rows<T, V>(th, dout, ldd, y, ldy, dy, lddy, npix, cw, ACT);
}

// Finalize kernels run as (32 channels x 32 parts) 1024-thread workgroups: part j sums partial blocks
// j, j+32, ... of its channel (128-byte coalesced rows), LDS combines the 32 parts; the thread with
// part 0 gets the totals and returns its channel, the others return -1.  (A one-thread-per-channel
// loop over 512 partials cost ~95 us per launch, 15 ms per training step.)
constexpr int FIN_CH = 16, FIN_PARTS = 64;
__device__ __forceinline__ int fin_reduce(const float* __restrict__ partial, int nblk, int C, double& s, double& q) {
    __shared__ double red[2][FIN_PARTS][FIN_CH + 1];
    const int cl = threadIdx.x & (FIN_CH - 1), part = threadIdx.x / FIN_CH;
    const int c = blockIdx.x * FIN_CH + cl;
    double ls = 0.0, lq = 0.0;
    if (c < C)
#pragma unroll 8
        for (int b = part; b < nblk; b += FIN_PARTS) {
            ls += partial[(long)b * 2 * C + c];
            lq += partial[(long)b * 2 * C + C + c];
        }
    red[0][part][cl] = ls;
    red[1][part][cl] = lq;
    __syncthreads();
    if (part != 0 || c >= C) return -1;
    s = 0.0; q = 0.0;
    for (int j = 0; j < FIN_PARTS; ++j) { s += red[0][j][cl]; q += red[1][j][cl]; }
    return c;
}

// finalize for training-mode BN, from the partial rows of k_channel_reduce
__global__ void k_bn_finalize(const float* __restrict__ partial, int nblk, float count, int C,
                              const void* __restrict__ gamma_, const void* __restrict__ beta_,
                              void* __restrict__ rmean_, void* __restrict__ rvar_, float momentum, float eps,
                              float* __restrict__ mean, float* __restrict__ invstd,
                              float* __restrict__ scale, float* __restrict__ shift, int pdt, int bdt) {
    const PIn gamma{gamma_, pdt}; const PIn beta{beta_, pdt}; const PIo rmean{rmean_, bdt}, rvar{rvar_, bdt};
    double s, q;
    const int c = fin_reduce(partial, nblk, C, s, q);
    if (c < 0) return;
    bn_fwd_publish(bn_fwd_coef(s, q, count, eps, gamma.ld(c), beta.ld(c)), c, momentum, mean, invstd, scale, shift, rmean, rvar);
}

__global__ void k_bn_eval_coeffs(const void* __restrict__ gamma_, const void* __restrict__ beta_,
                                 const void* __restrict__ rmean_, const void* __restrict__ rvar_, float eps,
                                 int C, float* __restrict__ scale, float* __restrict__ shift, int pdt, int bdt) {
    const PIn gamma{gamma_, pdt}; const PIn beta{beta_, pdt}; const PIn rmean{rmean_, bdt}, rvar{rvar_, bdt};
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float g = gamma.ld(c) / sqrtf(rvar.ld(c) + eps);
    scale[c] = g;
    shift[c] = beta.ld(c) - rmean.ld(c) * g;
}

// backward finalize, from the partial rows of k_channel_reduce: dgamma, dbeta, coef = [A, B, D] of bn_bwd_coef
__global__ void k_bn_bwd_finalize(const float* __restrict__ partial, int nblk, float count, int C,
                                  const void* __restrict__ gamma_, const float* __restrict__ mean, const float* __restrict__ invstd,
                                  void* __restrict__ dgamma_, void* __restrict__ dbeta_, float* __restrict__ coef, int pdt) {
    const PIn gamma{gamma_, pdt}; const PIo dgamma{dgamma_, pdt}, dbeta{dbeta_, pdt};
    double s, q;
    const int c = fin_reduce(partial, nblk, C, s, q);
    if (c < 0) return;
    const BnBwdCoef k = bn_bwd_coef(s, q, count, gamma, mean, invstd, c);
    dbeta.st(c, k.dbeta);
    dgamma.st(c, k.dgamma);
    coef[c] = k.A;
    coef[C + c] = k.B;
    coef[2 * C + c] = k.D;
}

__global__ void k_sum_finalize(const float* __restrict__ partial, int nblk, int C, float* __restrict__ out) {
    double s, q;
    const int c = fin_reduce(partial, nblk, C, s, q);
    if (c >= 0) out[c] = (float)s;
}

// out = act(y*scale + shift) (+ res)
template <typename T, int V>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_bn_act_fwd(const T* __restrict__ y, int ldy, const float* __restrict__ scale,
                             const float* __restrict__ shift, const T* __restrict__ res, int ldr,
                             T* __restrict__ out, int ldo, long npix, int cv, int act, int tpr) {
    const RsThread th = rs_thread(tpr, cv);
    if (!th.active) return;
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { sc[j] = scale[th.cg * V + j]; sh[j] = shift[th.cg * V + j]; }
    bn_act_fwd_rows<T, V>(th, y, ldy, res, ldr, out, ldo, npix, sc, sh, act);
}

// dy = A*dz + B*y + D with (A, B, D) = coef rows from k_bn_bwd_finalize; eval-style, frozen statistics (coef == null):
// (scale, 0, 0), dy = scale*dz
template <typename T, int V>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_bn_act_bwd_apply(const T* __restrict__ dout, int ldd, const T* __restrict__ y, int ldy,
                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                   const float* __restrict__ coef, T* __restrict__ dy, int lddy,
                                   long npix, int C, int act, int tpr) {
    const int cw = tpr * V;                                  // channels of this workgroup
    for (int t = threadIdx.x; t < cw; t += TPB) {
        const int c = blockIdx.y * cw + t;
        const bool in = c < C;
        cf[t] = in ? scale[c] : 0.f;
        cf[cw + t] = in ? shift[c] : 0.f;
        cf[2 * cw + t] = in ? (coef ? coef[c] : scale[c]) : 0.f;
        cf[3 * cw + t] = (in && coef) ? coef[C + c] : 0.f;
        cf[4 * cw + t] = (in && coef) ? coef[2 * C + c] : 0.f;
    }
    __syncthreads();
    const RsThread th = rs_thread(tpr, C / V);
    if (!th.active) return;
    bn_act_bwd_rows<T, V>(th, dout, ldd, y, ldy, dy, lddy, npix, cw, act);
}

// ---------------------------------------------------------------------------------------------
// SPPF 5x5 stride-1 pad-2 max pool; idx = kh*5+kw of the FIRST maximum in window scan order
// (ATen max_pool2d: strictly-greater update, NaN propagates) so ties route gradient identically.
// ---------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ void k_maxpool5_fwd(const T* __restrict__ x, int ldx, T* __restrict__ out, int ldo,
                               uint8_t* __restrict__ idx, int N, int H, int W, int C) {
    const int cv = C / V;
    long total = (long)N * H * W * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long p = i / cv;
        int cg = (int)(i - p * cv);
        int w = (int)(p % W);
        long t = p / W;
        int h = (int)(t % H);
        long n = t / H;
        float best[V];
        int bi[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { best[j] = -INFINITY; bi[j] = -1; }
        // a row of the window = five UNCONDITIONAL loads (clamped addresses) issued together, then the compare chain in
        // ATen's scan order on the taps that exist; the first form (a branch in front of each of the 25 loads) took 26 us
        // on the 6.5 MB SPPF maps
#pragma unroll
        for (int kh = 0; kh < 5; ++kh) {
            const int hh = h + kh - 2;
            const bool rok = hh >= 0 && hh < H;
            const int hc = hh < 0 ? 0 : (hh >= H ? H - 1 : hh);
            pack_t<T, V> raw[5];
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) {
                const int ww = w + kw - 2;
                const int wc = ww < 0 ? 0 : (ww >= W ? W - 1 : ww);
                raw[kw] = load_raw<T, V>(x + ((n * H + hc) * W + wc) * ldx + cg * V);
            }
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) {
                const int ww = w + kw - 2;
                if (!(rok && ww >= 0 && ww < W)) continue;
                float a[V];
                unpack<T, V>(raw[kw], a);
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (a[j] > best[j] || a[j] != a[j] || bi[j] < 0) { best[j] = a[j]; bi[j] = kh * 5 + kw; }
            }
        }
        store_pack<T, V>(out + p * ldo + cg * V, best);
        pack_t<uint8_t, V> pi;                                // the V argmax bytes in one store
#pragma unroll
        for (int j = 0; j < V; ++j) pi.v[j] = (uint8_t)bi[j];
        *reinterpret_cast<pack_t<uint8_t, V>*>(idx + p * C + cg * V) = pi;
    }
}

// gather form of the backward: dx(p) = sum over the <=25 windows containing p whose argmax is p
template <typename T, int V, bool ACC>
__global__ void k_maxpool5_bwd(const T* __restrict__ dout, int ldd, const uint8_t* __restrict__ idx,
                               T* __restrict__ dx, int ldx, int N, int H, int W, int C) {
    const int cv = C / V;
    long total = (long)N * H * W * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long p = i / cv;
        int cg = (int)(i - p * cv);
        int w = (int)(p % W);
        long t = p / W;
        int h = (int)(t % H);
        long n = t / H;
        float g[V];
#pragma unroll
        for (int j = 0; j < V; ++j) g[j] = 0.f;
#pragma unroll
        for (int kh = 0; kh < 5; ++kh) {
            const int oh = h - kh + 2;        // output row whose window tap kh lands on h
            const bool rok = oh >= 0 && oh < H;
            const int oc = oh < 0 ? 0 : (oh >= H ? H - 1 : oh);
            pack_t<T, V> raw[5];
            pack_t<uint8_t, V> ri[5];
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) {      // five unconditional (clamped) gradient + index loads per row, then the sums
                const int ow = w - kw + 2;
                const int wc = ow < 0 ? 0 : (ow >= W ? W - 1 : ow);
                const long q = (n * H + oc) * W + wc;
                raw[kw] = load_raw<T, V>(dout + q * ldd + cg * V);
                ri[kw] = *reinterpret_cast<const pack_t<uint8_t, V>*>(idx + q * C + cg * V);
            }
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) {
                const int ow = w - kw + 2;
                if (!(rok && ow >= 0 && ow < W)) continue;
                float d[V];
                unpack<T, V>(raw[kw], d);
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (ri[kw].v[j] == kh * 5 + kw) g[j] += d[j];
            }
        }
        if (ACC) {
            float b[V];
            load_pack<T, V>(dx + p * ldx + cg * V, b);
#pragma unroll
            for (int j = 0; j < V; ++j) g[j] += b[j];
        }
        store_pack<T, V>(dx + p * ldx + cg * V, g);
    }
}

// nearest x2 upsample: out(2H,2W); backward sums the 2x2 block
template <typename T, int V>
__global__ void k_upsample2x_fwd(const T* __restrict__ x, int ldx, T* __restrict__ out, int ldo,
                                 int N, int H, int W, int C) {
    const int cv = C / V;
    const int OW = 2 * W, OH = 2 * H;
    long total = (long)N * OH * OW * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long p = i / cv;
        int cg = (int)(i - p * cv);
        int ow = (int)(p % OW);
        long t = p / OW;
        int oh = (int)(t % OH);
        long n = t / OH;
        pack_t<T, V> v = *reinterpret_cast<const pack_t<T, V>*>(x + ((n * H + (oh >> 1)) * W + (ow >> 1)) * ldx + cg * V);
        *reinterpret_cast<pack_t<T, V>*>(out + p * ldo + cg * V) = v;
    }
}

template <typename T, int V, bool ACC>
__global__ void k_upsample2x_bwd(const T* __restrict__ dout, int ldd, T* __restrict__ dx, int ldx,
                                 int N, int H, int W, int C) {
    const int cv = C / V;
    const int OW = 2 * W, OH = 2 * H;
    long total = (long)N * H * W * cv;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long p = i / cv;
        int cg = (int)(i - p * cv);
        int w = (int)(p % W);
        long t = p / W;
        int h = (int)(t % H);
        long n = t / H;
        float g[V];
#pragma unroll
        for (int j = 0; j < V; ++j) g[j] = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float d[V];
                load_pack<T, V>(dout + ((n * OH + 2 * h + a) * OW + 2 * w + b) * ldd + cg * V, d);
#pragma unroll
                for (int j = 0; j < V; ++j) g[j] += d[j];
            }
        if (ACC) {
            float b2[V];
            load_pack<T, V>(dx + p * ldx + cg * V, b2);
#pragma unroll
            for (int j = 0; j < V; ++j) g[j] += b2[j];
        }
        store_pack<T, V>(dx + p * ldx + cg * V, g);
    }
}

// Workgroups along x of a row-strided kernel with tpr lanes per row: a workgroup takes RS_ROWS * rpb pixel rows per
// iteration; at most max(cap, cap_min) workgroups, and every workgroup gets the same number of iterations.
inline long rs_blocks(long npix, int tpr, long cap, long cap_min) {
    const int rpb = TPB / tpr;
    long units = (npix + (long)RS_ROWS * rpb - 1) / ((long)RS_ROWS * rpb);
    if (units < 1) units = 1;
    if (cap < cap_min) cap = cap_min;
    const long iters = (units + cap - 1) / cap;
    return (units + iters - 1) / iters;
}

// Launch plan of a row-strided kernel: x walks pixel rows, y covers the channel groups beyond one row.  At most RS_MAXBLK
// workgroups (all resident at once: no partial last round).
// narrow: the plan of the training-path BatchNorm kernels (the accumulator forms above).  Every workgroup pays a prologue /
// epilogue per channel it covers (16 accumulator loads + double arithmetic, or an LDS reduction + atomics), whatever
// the tensor's size: on a 20x20 map with 512 channels a workgroup that spans all channels (64 lanes per row) and two
// rows per lane fetched 32 KB of accumulators for 8 KB of activations.  Wide layers on small maps therefore use
// 16-lane rows (256-byte segments, channel groups on blockIdx.y): measured 12.1 -> 10.2 us forward and 30.6 -> 24.6 us
// backward for 512 channels at 20x20 x 32 images; capping the workgroup count as well made the 64..128-channel
// layers slower and is not done.
struct RsPlan { int tpr; dim3 grid; };
inline RsPlan rs_plan(long npix, int cv, bool narrow) {
    RsPlan p;
    p.tpr = cv < TPB ? cv : TPB;
    if (narrow && p.tpr > 16 && npix * cv <= (1L << 20)) p.tpr = 16;   // <= 8 M elements
    const int gy = ceil_div(cv, p.tpr);
    p.grid = dim3((unsigned)rs_blocks(npix, p.tpr, narrow ? RS_MAXBLK / gy : RS_MAXBLK, 8), (unsigned)gy);
    return p;
}

inline int ew_grid(long total) {
    long b = (total + TPB - 1) / TPB;
    return (int)(b < 1 ? 1 : (b > 256 * 16 ? 256 * 16 : b));   // <= 16 blocks per CU, grid-stride the rest
}

template <typename TI>
int ncm_to_nhwc_out(const void* src, long sn, long sc, long off, void* dst, int dst_dtype, int ld, int N,
                    int C, int HW, hipStream_t st) {
    dim3 g(ceil_div(HW, 32), ceil_div(C, 32), N);
    YOLO_DISPATCH_T(dst_dtype, hipLaunchKernelGGL((k_ncm_to_nhwc<TI, T>), g, dim3(256), 0, st, (const TI*)src,
                                                  sn, sc, off, (T*)dst, ld, C, HW));
    return YOLO_LAUNCH_CHECK();
}
template <typename TI>
int nhwc_to_ncm_out(const void* src, int ld, void* dst, int dst_dtype, long sn, long sc, long off, int N,
                    int C, int HW, hipStream_t st) {
    dim3 g(ceil_div(HW, 32), ceil_div(C, 32), N);
    YOLO_DISPATCH_T(dst_dtype, hipLaunchKernelGGL((k_nhwc_to_ncm<TI, T>), g, dim3(256), 0, st, (const TI*)src,
                                                  ld, (T*)dst, sn, sc, off, C, HW));
    return YOLO_LAUNCH_CHECK();
}

}  // namespace

#define PICK_V(T, ok, ...)                                       \
    if (ok) { constexpr int V = vec_of<T>::N; __VA_ARGS__; }     \
    else    { constexpr int V = 1; __VA_ARGS__; }
// the activation as a template parameter: no per-element select between SiLU and identity
#define PICK_ACT(act, ...)                                       \
    if (act) { constexpr int ACT = 1; __VA_ARGS__; }             \
    else     { constexpr int ACT = 0; __VA_ARGS__; }
// the instantiations of the channel reductions: MODE 0 has no activation
#define PICK_MODE_ACT(mode, act, ...)                            \
    if ((mode) == 0) { constexpr int MODE = 0, ACT = 0; __VA_ARGS__; } \
    else { constexpr int MODE = 1; PICK_ACT(act, __VA_ARGS__) }

extern "C" {

int yolo_memset0(void* p, size_t bytes, hipStream_t st) { return yolo_zero_async(p, bytes, st); }

int yolo_ncm_to_nhwc(const void* src, int src_dtype, long sn, long sc, long off, void* dst, int dst_dtype,
                     int ld, int N, int C, int HW, hipStream_t st) {
    switch (src_dtype) {
        case YOLO_F32:  return ncm_to_nhwc_out<float>(src, sn, sc, off, dst, dst_dtype, ld, N, C, HW, st);
        case YOLO_BF16: return ncm_to_nhwc_out<bf16_t>(src, sn, sc, off, dst, dst_dtype, ld, N, C, HW, st);
        case YOLO_F16:  return ncm_to_nhwc_out<f16_t>(src, sn, sc, off, dst, dst_dtype, ld, N, C, HW, st);
    }
    return YOLO_ERR_DTYPE;
}

// up to 8 NHWC branch tensors (one dtype) <-> preds (N, cp, M) of the same dtype: branch i occupies channels
// [c_off[i], c_off[i] + C[i]) and anchors [m_off[i], m_off[i] + HW[i]).  pack != 0: branches -> preds; 0: preds -> branches.
int yolo_head_group(int pack, int n, void* const* branches, const int* lds, const int* Cs, const int* HWs, const int* c_offs,
                    const int* m_offs, void* preds, int cp, int M, int N, int dtype, hipStream_t st) {
    if (n < 1 || n > HEAD_GROUP) return YOLO_ERR_ARG;
    HeadGroup g;
    int wgs = 0;
    for (int i = 0; i < HEAD_GROUP; ++i) {
        const int j = i < n ? i : 0;
        g.t[i] = branches[j]; g.ld[i] = lds[j]; g.C[i] = Cs[j]; g.HW[i] = HWs[j]; g.c_off[i] = c_offs[j]; g.m_off[i] = m_offs[j];
        g.tp[i] = ceil_div(HWs[j], 32);
        g.start[i] = wgs;
        if (i < n) wgs += g.tp[i] * ceil_div(Cs[j], 32);
    }
    g.start[HEAD_GROUP] = wgs;
    g.n = n;
    if (wgs == 0 || N == 0) return YOLO_OK;
    // 16-bit tensors with 8-element alignment everywhere: the 16-byte form, 64 pixels x all channels per workgroup
    bool vec = dtype != YOLO_F32 && M % 8 == 0 && (reinterpret_cast<uintptr_t>(preds) & 15) == 0;
    int cmax = 0;
    for (int i = 0; i < n && vec; ++i) {
        vec = Cs[i] % 8 == 0 && HWs[i] % 8 == 0 && m_offs[i] % 8 == 0 && lds[i] % 8 == 0 && (reinterpret_cast<uintptr_t>(branches[i]) & 15) == 0;
        cmax = Cs[i] > cmax ? Cs[i] : cmax;
    }
    if (vec && (size_t)64 * (cmax + 2) * 2 <= 48 * 1024) {
        int w2 = 0;
        for (int i = 0; i < HEAD_GROUP; ++i) {
            const int j = i < n ? i : 0;
            g.start[i] = w2;
            if (i < n) w2 += ceil_div(HWs[j], 64);
        }
        g.start[HEAD_GROUP] = w2;
        const dim3 grid2((unsigned)w2, (unsigned)N);
        const size_t lds_bytes = (size_t)64 * (cmax + 2) * 2;
        if (dtype == YOLO_BF16) {
            if (pack) hipLaunchKernelGGL((k_head_group_vec<bf16_t, true>), grid2, dim3(256), lds_bytes, st, g, (bf16_t*)preds, (long)cp * M, (long)M);
            else hipLaunchKernelGGL((k_head_group_vec<bf16_t, false>), grid2, dim3(256), lds_bytes, st, g, (bf16_t*)preds, (long)cp * M, (long)M);
        } else {
            if (pack) hipLaunchKernelGGL((k_head_group_vec<f16_t, true>), grid2, dim3(256), lds_bytes, st, g, (f16_t*)preds, (long)cp * M, (long)M);
            else hipLaunchKernelGGL((k_head_group_vec<f16_t, false>), grid2, dim3(256), lds_bytes, st, g, (f16_t*)preds, (long)cp * M, (long)M);
        }
        return YOLO_LAUNCH_CHECK();
    }
    const dim3 grid((unsigned)wgs, (unsigned)N);
    YOLO_DISPATCH_T(dtype, {
        if (pack) hipLaunchKernelGGL((k_head_group<T, true>), grid, dim3(256), 0, st, g, (T*)preds, (long)cp * M, (long)M);
        else hipLaunchKernelGGL((k_head_group<T, false>), grid, dim3(256), 0, st, g, (T*)preds, (long)cp * M, (long)M);
    });
    return YOLO_LAUNCH_CHECK();
}

int yolo_nhwc_to_ncm(const void* src, int src_dtype, int ld, void* dst, int dst_dtype, long sn, long sc,
                     long off, int N, int C, int HW, hipStream_t st) {
    switch (src_dtype) {
        case YOLO_F32:  return nhwc_to_ncm_out<float>(src, ld, dst, dst_dtype, sn, sc, off, N, C, HW, st);
        case YOLO_BF16: return nhwc_to_ncm_out<bf16_t>(src, ld, dst, dst_dtype, sn, sc, off, N, C, HW, st);
        case YOLO_F16:  return nhwc_to_ncm_out<f16_t>(src, ld, dst, dst_dtype, sn, sc, off, N, C, HW, st);
    }
    return YOLO_ERR_DTYPE;
}

int yolo_copy_channels(const void* src, int ld_src, void* dst, int ld_dst, long npix, int C, int accumulate,
                       int dtype, hipStream_t st) {
    if (npix <= 0 || C <= 0) return YOLO_OK;
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(src, ld_src, C) && vec_ok<T>(dst, ld_dst, C);
        PICK_V(T, ok, {
            int cv = C / V;
            int g = ew_grid(npix * cv);
            if (accumulate)
                hipLaunchKernelGGL((k_copy_channels<T, V, true>), dim3(g), dim3(TPB), 0, st, (const T*)src, ld_src,
                                   (T*)dst, ld_dst, npix, cv);
            else
                hipLaunchKernelGGL((k_copy_channels<T, V, false>), dim3(g), dim3(TPB), 0, st, (const T*)src, ld_src,
                                   (T*)dst, ld_dst, npix, cv);
        });
    });
    return YOLO_LAUNCH_CHECK();
}

// dst[p][c] = src0 + src1 (+ src2 (+ src3)); every operand an NHWC channel slice with its own row stride; dst may be one
// of the sources.  Replaces autograd's gradient accumulation at fan-out points (model_blocks.py:62,92,156,223-224, neck.py:41-44)
int yolo_add_n(const void* s0, int ld0, const void* s1, int ld1, const void* s2, int ld2, const void* s3, int ld3, int nsrc,
               void* dst, int ld_dst, long npix, int C, int dtype, hipStream_t st) {
    if (nsrc < 2 || nsrc > 4 || npix <= 0) return nsrc >= 2 && nsrc <= 4 ? YOLO_OK : YOLO_ERR_ARG;
    AddSrcs a;
    a.p[0] = s0; a.p[1] = s1; a.p[2] = s2; a.p[3] = s3;
    a.ld[0] = ld0; a.ld[1] = ld1; a.ld[2] = ld2; a.ld[3] = ld3;
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(dst, ld_dst, C);
        for (int k = 0; k < nsrc; ++k) ok = ok && vec_ok<T>(a.p[k], a.ld[k], C);
        PICK_V(T, ok, {
            int cv = C / V;
            int g = ew_grid(npix * cv);
            if (nsrc == 2) hipLaunchKernelGGL((k_add_n<T, V, 2>), dim3(g), dim3(TPB), 0, st, a, (T*)dst, ld_dst, npix, cv);
            else if (nsrc == 3) hipLaunchKernelGGL((k_add_n<T, V, 3>), dim3(g), dim3(TPB), 0, st, a, (T*)dst, ld_dst, npix, cv);
            else hipLaunchKernelGGL((k_add_n<T, V, 4>), dim3(g), dim3(TPB), 0, st, a, (T*)dst, ld_dst, npix, cv);
        });
    });
    return YOLO_LAUNCH_CHECK();
}

// number of partial blocks yolo_bn_stats / yolo_bn_act_bwd_reduce will write for this problem
int yolo_reduce_nblk(long npix, int C) {
    // one partial row per workgroup; same balanced sizing as the other row-strided kernels (<= 1024 workgroups)
    const int cv = C / 8 > 0 ? C / 8 : 1;
    long cap = npix / 32;              // keep the partial rows (2*C floats each) well below the tensor's own bytes
    if (cap > 1024) cap = 1024;
    return (int)rs_blocks(npix, cv < TPB ? cv : TPB, cap, 1);
}

static int launch_reduce(int mode, const void* y, int ldy, const void* dout, int ldd, const float* scale,
                         const float* shift, long npix, int C, int act, int dtype, float* partial, int nblk, hipStream_t st) {
    if (nblk != yolo_reduce_nblk(npix, C)) return YOLO_ERR_ARG;
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(y, ldy, C) && (mode == 0 || vec_ok<T>(dout, ldd, C));
        PICK_V(T, ok, {
            const RsPlan pl = rs_plan(npix, C / V, false);
            PICK_MODE_ACT(mode, act, hipLaunchKernelGGL((k_channel_reduce<T, V, MODE, ACT>), dim3(nblk, pl.grid.y), dim3(TPB), 0, st,
                                                        (const T*)y, ldy, (const T*)dout, ldd, scale, shift, npix, C, partial, pl.tpr));
        });
    });
    return YOLO_LAUNCH_CHECK();
}

int yolo_bn_stats(const void* y, int ldy, long npix, int C, int dtype, float* partial, int nblk, hipStream_t st) {
    return launch_reduce(0, y, ldy, nullptr, 0, nullptr, nullptr, npix, C, 0, dtype, partial, nblk, st);
}

int yolo_bn_finalize(const float* partial, int nblk, long count, int C, const void* gamma, const void* beta,
                     void* running_mean, void* running_var, float momentum, float eps, float* mean,
                     float* invstd, float* scale, float* shift, int pdtype, int bdtype, hipStream_t st) {
    if (!pdt_ok(pdtype) || !pdt_ok(bdtype)) return YOLO_ERR_DTYPE;
    hipLaunchKernelGGL(k_bn_finalize, dim3(ceil_div(C, FIN_CH)), dim3(FIN_CH * FIN_PARTS), 0, st, partial, nblk, (float)count, C,
                       gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift, pdtype, bdtype);
    return YOLO_LAUNCH_CHECK();
}

int yolo_bn_eval_coeffs(const void* gamma, const void* beta, const void* running_mean, const void* running_var,
                        float eps, int C, float* scale, float* shift, int pdtype, int bdtype, hipStream_t st) {
    if (!pdt_ok(pdtype) || !pdt_ok(bdtype)) return YOLO_ERR_DTYPE;
    hipLaunchKernelGGL(k_bn_eval_coeffs, dim3(ceil_div(C, 128)), dim3(128), 0, st, gamma, beta, running_mean, running_var, eps, C,
                       scale, shift, pdtype, bdtype);
    return YOLO_LAUNCH_CHECK();
}

int yolo_sum_finalize(const float* partial, int nblk, int C, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_sum_finalize, dim3(ceil_div(C, FIN_CH)), dim3(FIN_CH * FIN_PARTS), 0, st, partial, nblk, C, out);
    return YOLO_LAUNCH_CHECK();
}

int yolo_bn_act_fwd(const void* y, int ldy, const float* scale, const float* shift, const void* res, int ldres,
                    void* out, int ldout, long npix, int C, int act, int dtype, hipStream_t st) {
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(y, ldy, C) && vec_ok<T>(out, ldout, C) && (!res || vec_ok<T>(res, ldres, C));
        PICK_V(T, ok, {
            const RsPlan pl = rs_plan(npix, C / V, false);
            hipLaunchKernelGGL((k_bn_act_fwd<T, V>), pl.grid, dim3(TPB), 0, st, (const T*)y, ldy, scale,
                               shift, (const T*)res, ldres, (T*)out, ldout, npix, C / V, act, pl.tpr);
        });
    });
    return YOLO_LAUNCH_CHECK();
}

int yolo_bn_act_bwd_reduce(const void* dout, int ldd, const void* y, int ldy, const float* scale, const float* shift,
                           const float* mean, const float* invstd, long npix, int C, int act, int dtype,
                           float* partial, int nblk, hipStream_t st) {
    return launch_reduce(1, y, ldy, dout, ldd, scale, shift, npix, C, act, dtype, partial, nblk, st);
}

int yolo_bn_bwd_finalize(const float* partial, int nblk, long count, int C, const void* gamma, const float* mean,
                         const float* invstd, void* dgamma, void* dbeta, float* coef, int pdtype, hipStream_t st) {
    if (!pdt_ok(pdtype)) return YOLO_ERR_DTYPE;
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3(ceil_div(C, FIN_CH)), dim3(FIN_CH * FIN_PARTS), 0, st, partial, nblk,
                       (float)count, C, gamma, mean, invstd, dgamma, dbeta, coef, pdtype);
    return YOLO_LAUNCH_CHECK();
}

int yolo_bn_act_bwd_apply(const void* dout, int ldd, const void* y, int ldy, const float* scale, const float* shift,
                          const float* mean, const float* invstd, const float* coef, void* dy, int lddy, long npix,
                          int C, int act, int dtype, hipStream_t st) {
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(y, ldy, C) && vec_ok<T>(dout, ldd, C) && vec_ok<T>(dy, lddy, C);
        PICK_V(T, ok, {
            const RsPlan pl = rs_plan(npix, C / V, false);
            hipLaunchKernelGGL((k_bn_act_bwd_apply<T, V>), pl.grid, dim3(TPB), 5 * pl.tpr * V * sizeof(float), st, (const T*)dout,
                               ldd, (const T*)y, ldy, scale, shift, coef, (T*)dy, lddy, npix, C, act, pl.tpr);
        });
    });
    return YOLO_LAUNCH_CHECK();
}

// ---- accumulator form (no finalize launches).  acc: fp32 [YOLO_BN_REPL = 8][2][C], zeroed by the caller.
int yolo_bn_acc_elems(int C) { return BN_REPL * 2 * C; }

static int launch_acc(int mode, const void* y, int ldy, const void* dout, int ldd, const float* scale, const float* shift,
                      long npix, int C, int act, int dtype, float* acc, hipStream_t st) {
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(y, ldy, C) && (mode == 0 || vec_ok<T>(dout, ldd, C));
        PICK_V(T, ok, {
            const RsPlan pl = rs_plan(npix, C / V, true);
            PICK_MODE_ACT(mode, act, hipLaunchKernelGGL((k_channel_acc<T, V, MODE, ACT>), pl.grid, dim3(TPB), 0, st, (const T*)y, ldy,
                                                        (const T*)dout, ldd, scale, shift, npix, C, acc, pl.tpr));
        });
    });
    return YOLO_LAUNCH_CHECK();
}

int yolo_bn_stats_acc(const void* y, int ldy, long npix, int C, int dtype, float* acc, hipStream_t st) {
    return launch_acc(0, y, ldy, nullptr, 0, nullptr, nullptr, npix, C, 0, dtype, acc, st);
}

int yolo_bn_finalize_acc(const float* acc, long count, int C, const void* gamma, const void* beta, void* running_mean,
                         void* running_var, float momentum, float eps, float* mean, float* invstd, float* scale,
                         float* shift, int pdtype, int bdtype, hipStream_t st) {
    if (!pdt_ok(pdtype) || !pdt_ok(bdtype)) return YOLO_ERR_DTYPE;
    hipLaunchKernelGGL(k_bn_finalize_acc, dim3(ceil_div(C, 64)), dim3(64), 0, st, acc, (float)count, C, gamma, beta,
                       running_mean, running_var, momentum, eps, mean, invstd, scale, shift, pdtype, bdtype);
    return YOLO_LAUNCH_CHECK();
}

int yolo_bn_act_fwd_train(const void* y, int ldy, const float* acc, long count, const void* gamma, const void* beta,
                          void* running_mean, void* running_var, float momentum, float eps, float* mean, float* invstd,
                          float* scale, float* shift, const void* res, int ldres, void* out, int ldout, long npix, int C,
                          int act, int dtype, int pdtype, int bdtype, hipStream_t st) {
    if (!pdt_ok(pdtype) || !pdt_ok(bdtype)) return YOLO_ERR_DTYPE;
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(y, ldy, C) && vec_ok<T>(out, ldout, C) && (!res || vec_ok<T>(res, ldres, C));
        PICK_V(T, ok, {
            const RsPlan pl = rs_plan(npix, C / V, true);
            PICK_ACT(act, hipLaunchKernelGGL((k_bn_act_fwd_train<T, V, ACT>), pl.grid, dim3(TPB), 2 * pl.tpr * V * sizeof(float), st,
                               (const T*)y, ldy, acc, (float)count, gamma, beta, running_mean, running_var, momentum, eps,
                               mean, invstd, scale, shift, (const T*)res, ldres, (T*)out, ldout, npix, C, pl.tpr, pdtype, bdtype));
        });
    });
    return YOLO_LAUNCH_CHECK();
}

// backward pass 1 with atomics: acc[8][2][C] (zeroed by the caller) += (sum dz, sum dz*y), dz = dout*act'(y*scale+shift)
int yolo_bn_bwd_reduce_acc(const void* dout, int ldd, const void* y, int ldy, const float* scale, const float* shift,
                           long npix, int C, int act, int dtype, float* acc, hipStream_t st) {
    return launch_acc(1, y, ldy, dout, ldd, scale, shift, npix, C, act, dtype, acc, st);
}

int yolo_bn_act_bwd_apply_train(const void* dout, int ldd, const void* y, int ldy, const float* scale, const float* shift,
                                const void* gamma, const float* mean, const float* invstd, const float* acc, long count,
                                void* dgamma, void* dbeta, void* dy, int lddy, long npix, int C, int act, int dtype,
                                int pdtype, hipStream_t st) {
    if (!pdt_ok(pdtype)) return YOLO_ERR_DTYPE;
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(y, ldy, C) && vec_ok<T>(dout, ldd, C) && vec_ok<T>(dy, lddy, C);
        PICK_V(T, ok, {
            const RsPlan pl = rs_plan(npix, C / V, true);
            PICK_ACT(act, hipLaunchKernelGGL((k_bn_act_bwd_apply_train<T, V, ACT>), pl.grid, dim3(TPB), 5 * pl.tpr * V * sizeof(float), st,
                               (const T*)dout, ldd, (const T*)y, ldy, scale, shift, gamma, mean, invstd, acc, (float)count,
                               dgamma, dbeta, (T*)dy, lddy, npix, C, pl.tpr, pdtype));
        });
    });
    return YOLO_LAUNCH_CHECK();
}

int yolo_maxpool5_fwd(const void* x, int ldx, void* out, int ldo, uint8_t* idx, int N, int H, int W, int C,
                      int dtype, hipStream_t st) {
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(x, ldx, C) && vec_ok<T>(out, ldo, C);
        PICK_V(T, ok, {
            hipLaunchKernelGGL((k_maxpool5_fwd<T, V>), dim3(ew_grid((long)N * H * W * (C / V))), dim3(TPB), 0, st,
                               (const T*)x, ldx, (T*)out, ldo, idx, N, H, W, C);
        });
    });
    return YOLO_LAUNCH_CHECK();
}

int yolo_maxpool5_bwd(const void* dout, int ldd, const uint8_t* idx, void* dx, int ldx, int N, int H, int W, int C,
                      int accumulate, int dtype, hipStream_t st) {
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(dout, ldd, C) && vec_ok<T>(dx, ldx, C);
        PICK_V(T, ok, {
            int g = ew_grid((long)N * H * W * (C / V));
            if (accumulate)
                hipLaunchKernelGGL((k_maxpool5_bwd<T, V, true>), dim3(g), dim3(TPB), 0, st, (const T*)dout, ldd, idx,
                                   (T*)dx, ldx, N, H, W, C);
            else
                hipLaunchKernelGGL((k_maxpool5_bwd<T, V, false>), dim3(g), dim3(TPB), 0, st, (const T*)dout, ldd, idx,
                                   (T*)dx, ldx, N, H, W, C);
        });
    });
    return YOLO_LAUNCH_CHECK();
}

int yolo_upsample2x_fwd(const void* x, int ldx, void* out, int ldo, int N, int H, int W, int C, int dtype,
                        hipStream_t st) {
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(x, ldx, C) && vec_ok<T>(out, ldo, C);
        PICK_V(T, ok, {
            hipLaunchKernelGGL((k_upsample2x_fwd<T, V>), dim3(ew_grid((long)N * 4 * H * W * (C / V))), dim3(TPB), 0, st,
                               (const T*)x, ldx, (T*)out, ldo, N, H, W, C);
        });
    });
    return YOLO_LAUNCH_CHECK();
}

int yolo_upsample2x_bwd(const void* dout, int ldd, void* dx, int ldx, int N, int H, int W, int C, int accumulate,
                        int dtype, hipStream_t st) {
    YOLO_DISPATCH_T(dtype, {
        bool ok = vec_ok<T>(dout, ldd, C) && vec_ok<T>(dx, ldx, C);
        PICK_V(T, ok, {
            int g = ew_grid((long)N * H * W * (C / V));
            if (accumulate)
                hipLaunchKernelGGL((k_upsample2x_bwd<T, V, true>), dim3(g), dim3(TPB), 0, st, (const T*)dout, ldd,
                                   (T*)dx, ldx, N, H, W, C);
            else
                hipLaunchKernelGGL((k_upsample2x_bwd<T, V, false>), dim3(g), dim3(TPB), 0, st, (const T*)dout, ldd,
                                   (T*)dx, ldx, N, H, W, C);
        });
    });
    return YOLO_LAUNCH_CHECK();
}

}  // extern "C"
