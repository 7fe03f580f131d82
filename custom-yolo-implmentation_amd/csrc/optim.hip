// AdamW step of ALL parameters in one launch.
// torch.optim.AdamW semantics (decoupled weight decay, bias correction, eps added to sqrt(v)/sqrt(bc2)):
//   p *= 1 - lr*wd;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// As computed (adam_elem): the decay and the subtraction are ONE fused multiply-add, p = fma(p, 1 - lr*wd, -step), so the
// decayed parameter is never rounded on its own; sqrt is the hardware root (within 1 ulp, not correctly rounded).
// A device job table lists (param, grad, exp_avg, exp_avg_sq, numel) per tensor; one workgroup owns one 4096-element
// chunk of one tensor (job found once per workgroup).  Hyper-parameters and the step counter live in device memory so
// a captured step follows a learning-rate schedule without recapture; GradScaler's scale / found_inf pair is
// honoured like torch's fused optimizers do (skip the whole step on overflow, unscale the gradient in flight).
// Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) rides on the same table: k_grad_sqnorm
// leaves one partial sum of squares per chunk, k_clip_finalize turns them into [total_norm, coef] in device memory and
// k_adamw multiplies the gradient by coef in flight, next to the unscale (the .grad tensors are not modified).
// Exponential moving average of the weights (the ModelEMA of the YOLOv5 / v8 recipes; the reference has none) rides in
// k_adamw too: a record may carry an fp32 shadow `e` and a control block ectl = [decay, tau, updates] (doubles, device
// memory, one per parameter group); with d = tau > 0 ? decay * (1 - exp(-updates / tau)) : decay the kernel leaves
// e = d*e + (1-d)*w behind, w being the parameter AS STORED.  k_adamw_tick counts `updates` next to `step`, so a step
// skipped on found_inf moves neither the shadows nor the ramp.  k_ema_lerp is the same average over tensors that the
// optimizer does not step (BatchNorm running statistics): one more launch over a table of its own.
#include "common.h"

struct AdamJob {
    void* p;            // parameter, p_dtype
    const void* g;      // gradient, g_dtype
    float* m;           // exp_avg (fp32)
    float* v;           // exp_avg_sq (fp32)
    long n;             // elements
    long cstart;        // first 4096-element chunk (= workgroup) of this job
    int p_dtype, g_dtype;
    float* e;           // EMA shadow of p (fp32), or null
    double* ectl;       // EMA control block of the group [decay, tau, updates], or null
};

namespace {

constexpr int CHUNK = 4096;

template <typename P> __device__ __forceinline__ float ldf(const void* p, long i) { return to_f<P>(((const P*)p)[i]); }
__device__ __forceinline__ float ld_any(const void* p, int dt, long i) {
    return dt == YOLO_F32 ? ldf<float>(p, i) : dt == YOLO_BF16 ? ldf<bf16_t>(p, i) : ldf<f16_t>(p, i);
}
__device__ __forceinline__ void st_any(void* p, int dt, long i, float x) {
    if (dt == YOLO_F32) ((float*)p)[i] = x;
    else if (dt == YOLO_BF16) ((bf16_t*)p)[i] = from_f<bf16_t>(x);
    else ((f16_t*)p)[i] = from_f<f16_t>(x);
}

// The update of ONE element, shared by the packet path and the any-dtype path, so that the same (p, g, m, v) give the
// same bits whichever path a tensor takes (a low-precision gradient of an fp32 master goes through the generic one;
// left to the compiler the two loops were contracted differently: 1-ulp differences between the sharded runner and
// torch FSDP2 on the same gradients).  What the spelling does and does not pin: the two __fmaf_rn are fused
// multiply-adds wherever they are inlined, and their addends, the root and the divisions are operations that the
// compiler has nothing to contract with.  The LAST line is not pinned: without OCML_BASIC_ROUNDED_OPERATIONS
// __fsub_rn(x, y) is x - y and __fmul_rn(x, y) is x * y, and under the default contraction p*decay - step is compiled
// to ONE fused multiply-add on both paths (v_pk_fma_f32 with neg_lo / neg_hi on the addend in the packet loop,
// v_fma_f32 with a negated addend in the any-dtype loop): one rounding for the decay and the subtraction together, the
// decayed parameter is never rounded on its own.  That both loops agree there is the compiler's choice, held by
// tests/test_gpu_adamw.py's bit-for-bit comparison of the two paths.  (Spelled as __fmaf_rn(p, decay, -step) the line
// gives the same values but another instruction stream -- the negation moves into the step_size * m multiply -- so it
// stays as it is.)  __fsqrt_rn is the hardware square root between two v_ldexp_f32, no correction step: within 1 ulp
// (ISA manual), not correctly rounded.  tests/strict_optim.py counts these roundings and bounds every element by them.
__device__ __forceinline__ void adam_elem(float& p, float gg, float& m, float& v, float b1, float omb1, float b2, float omb2,
                                          float step_size, float bc2s, float decay, float eps) {
    m = __fmaf_rn(b1, m, __fmul_rn(omb1, gg));
    v = __fmaf_rn(b2, v, __fmul_rn(__fmul_rn(omb2, gg), gg));
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), bc2s), eps);
    p = __fsub_rn(__fmul_rn(p, decay), __fdiv_rn(__fmul_rn(step_size, m), denom));
}

// The EMA coefficients of one launch from the control block: df = fl(d), omd = fl(1 - d), both rounded from the double d.
__device__ __forceinline__ void ema_coef(const double* ectl, float& df, float& omd) {
    const double decay = ectl[0], tau = ectl[1], updates = ectl[2];
    const double d = tau > 0.0 ? decay * (1.0 - exp(-updates / tau)) : decay;
    df = (float)d;
    omd = (float)(1.0 - d);
}

// The job that owns this workgroup's chunk: the last record with cstart <= blockIdx.x (one thread per workgroup asks).
__device__ __forceinline__ int job_of_block(const AdamJob* __restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].cstart <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The EMA tail of the step kernels and k_ema_lerp: e = d*e + (1-d)*w, w the parameter AS STORED (as_stored: a bf16 / f16
// parameter's rounded value, so the average is one of the observable weights).
__device__ __forceinline__ float ema_elem(float e, float w, float df, float omd) { return __fmaf_rn(df, e, __fmul_rn(omd, w)); }
__device__ __forceinline__ float as_stored(float x, int dt) {
    return dt == YOLO_F32 ? x : dt == YOLO_BF16 ? to_f<bf16_t>(from_f<bf16_t>(x)) : to_f<f16_t>(from_f<f16_t>(x));
}
__device__ __forceinline__ void ema_packet(float* __restrict__ ema, long i, const float* w, float df, float omd) {
    float4 e = *reinterpret_cast<float4*>(ema + i);
    float* ep = &e.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) ep[k] = ema_elem(ep[k], w[k], df, omd);
    *reinterpret_cast<float4*>(ema + i) = e;
}

// step += 1 (and the group's EMA update count, found through the first record) unless the scaler found an overflow
// (one thread; the main kernel reads the updated values)
__global__ void k_adamw_tick(float* __restrict__ step, const float* __restrict__ found_inf, const AdamJob* __restrict__ jobs) {
    if (found_inf == nullptr || *found_inf == 0.f) {
        *step += 1.f;
        double* ectl = jobs[0].ectl;
        if (ectl != nullptr) ectl[2] += 1.0;
    }
}

// hyper = [lr, beta1, beta2, eps, weight_decay] as DOUBLES: 1 - beta and the bias corrections are formed in double
// like torch does on the host (1 - 0.999 in fp32 is off by 5e-5 relative, which shows in exp_avg_sq)
__global__ __launch_bounds__(256) void k_adamw(const AdamJob* __restrict__ jobs, int njobs, const double* __restrict__ hyper,
                                               const float* __restrict__ step, const float* __restrict__ grad_scale,
                                               const float* __restrict__ found_inf, const float* __restrict__ clip) {
    if (found_inf != nullptr && *found_inf != 0.f) return;
    __shared__ int sj;
    __shared__ float sc[9];                     // b1, 1-b1, b2, 1-b2, step_size, 1/sqrt(bc2), decay, ema d, ema 1-d
    if (threadIdx.x == 0) {
        const int lo = sj = job_of_block(jobs, njobs);
        const double lr = hyper[0], b1d = hyper[1], b2d = hyper[2], wd = hyper[4], t = (double)*step;
        const double bc1 = 1.0 - pow(b1d, t), bc2 = 1.0 - pow(b2d, t);
        sc[0] = (float)b1d; sc[1] = (float)(1.0 - b1d); sc[2] = (float)b2d; sc[3] = (float)(1.0 - b2d);
        sc[4] = (float)(lr / bc1); sc[5] = (float)sqrt(bc2); sc[6] = (float)(1.0 - lr * wd);
        sc[7] = 0.f; sc[8] = 0.f;
        if (jobs[lo].e != nullptr && jobs[lo].ectl != nullptr) ema_coef(jobs[lo].ectl, sc[7], sc[8]);
    }
    __syncthreads();
    const AdamJob j = jobs[sj];
    const float b1 = sc[0], omb1 = sc[1], b2 = sc[2], omb2 = sc[3], step_size = sc[4], bc2s = sc[5], decay = sc[6];
    const float eps = (float)hyper[3];
    const float df = sc[7], omd = sc[8];
    float* const ema = j.ectl != nullptr ? j.e : nullptr;
    float gs = grad_scale ? 1.f / *grad_scale : 1.f;            // GradScaler: gradients arrive multiplied by the scale
    if (clip != nullptr) gs *= clip[2];                         // clip state = [max_norm, total_norm, coef]; x * 1.f is x
    const long base = ((long)blockIdx.x - j.cstart) * CHUNK;
    if (j.p_dtype == YOLO_F32 && j.g_dtype == YOLO_F32 && (j.n & 3) == 0 &&
        ((reinterpret_cast<uintptr_t>(j.p) | reinterpret_cast<uintptr_t>(j.g) | reinterpret_cast<uintptr_t>(j.m) |
          reinterpret_cast<uintptr_t>(j.v) | reinterpret_cast<uintptr_t>(ema)) & 15) == 0) {
        // the common case: fp32 master weights and gradients, 16-byte packets
        for (long i = base + threadIdx.x * 4L; i < base + CHUNK && i < j.n; i += 256 * 4) {
            float4 p = *reinterpret_cast<float4*>((float*)j.p + i);
            const float4 g = *reinterpret_cast<const float4*>((const float*)j.g + i);
            float4 m = *reinterpret_cast<float4*>(j.m + i), v = *reinterpret_cast<float4*>(j.v + i);
            float* pp = &p.x; const float* gp = &g.x; float* mp = &m.x; float* vp = &v.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) adam_elem(pp[k], gp[k] * gs, mp[k], vp[k], b1, omb1, b2, omb2, step_size, bc2s, decay, eps);
            *reinterpret_cast<float4*>((float*)j.p + i) = p;
            *reinterpret_cast<float4*>(j.m + i) = m;
            *reinterpret_cast<float4*>(j.v + i) = v;
            if (ema != nullptr) ema_packet(ema, i, pp, df, omd);
        }
        return;
    }
    for (long i = base + threadIdx.x; i < base + CHUNK && i < j.n; i += 256) {
        float pv = ld_any(j.p, j.p_dtype, i), m = j.m[i], v = j.v[i];
        adam_elem(pv, ld_any(j.g, j.g_dtype, i) * gs, m, v, b1, omb1, b2, omb2, step_size, bc2s, decay, eps);
        j.m[i] = m;
        j.v[i] = v;
        st_any(j.p, j.p_dtype, i, pv);
        if (ema != nullptr) ema[i] = ema_elem(ema[i], as_stored(pv, j.p_dtype), df, omd);
    }
}

// ---- SGD with momentum (torch.optim.SGD: dampening 0, coupled weight decay, optional Nesterov, maximize False) over the
// same job table, v null and m the momentum buffer:
//   d = wd*p + g*gs;  buf = mu*buf + d;  n = nesterov ? mu*buf + d : buf;  p = p - lr*n
// Four fused multiply-adds and the unscale: one rounding each.  A zero buffer makes the first step buf = d, as torch's
// clone does.  The packet path and the any-dtype path share it, so identical inputs give identical bits on either.
__device__ __forceinline__ void sgd_elem(float& p, float g, float gs, float& buf, float lr, float mu, float wd, bool nesterov) {
    const float d = __fmaf_rn(wd, p, __fmul_rn(g, gs));
    buf = __fmaf_rn(mu, buf, d);
    const float n = nesterov ? __fmaf_rn(mu, buf, d) : buf;
    p = __fmaf_rn(-lr, n, p);
}

// hyper = [lr, momentum, weight_decay, nesterov (0 / 1), warmup_steps W, warmup_momentum mu0, warmup_lr_scale s0] as DOUBLES.
// Warm-up, per iteration and on the device: with t = *step after the tick (1, 2, ...) and f = (t - 1) / W, a step with
// t <= W runs at lr*(s0 + (1 - s0)*f) and mu0 + (mu - mu0)*f; later steps and W = 0 see lr and mu themselves.  A step
// skipped on found_inf does not tick, so it does not advance the warm-up either.
__global__ __launch_bounds__(256) void k_sgd(const AdamJob* __restrict__ jobs, int njobs, const double* __restrict__ hyper,
                                             const float* __restrict__ step, const float* __restrict__ grad_scale,
                                             const float* __restrict__ found_inf, const float* __restrict__ clip) {
    if (found_inf != nullptr && *found_inf != 0.f) return;
    __shared__ int sj;
    __shared__ float sc[5];                     // lr_t, mu_t, wd, ema d, ema 1-d
    if (threadIdx.x == 0) {
        const int lo = sj = job_of_block(jobs, njobs);
        double lr = hyper[0], mu = hyper[1];
        const double W = hyper[4], mu0 = hyper[5], s0 = hyper[6], t = (double)*step;
        if (W > 0.0 && t <= W) {
            const double f = (t - 1.0) / W;
            lr = lr * (s0 + (1.0 - s0) * f);
            mu = mu0 + (mu - mu0) * f;
        }
        sc[0] = (float)lr; sc[1] = (float)mu; sc[2] = (float)hyper[2];
        sc[3] = 0.f; sc[4] = 0.f;
        if (jobs[lo].e != nullptr && jobs[lo].ectl != nullptr) ema_coef(jobs[lo].ectl, sc[3], sc[4]);
    }
    __syncthreads();
    const AdamJob j = jobs[sj];
    const float lr = sc[0], mu = sc[1], wd = sc[2], df = sc[3], omd = sc[4];
    const bool nesterov = hyper[3] != 0.0;
    float* const ema = j.ectl != nullptr ? j.e : nullptr;
    float gs = grad_scale ? 1.f / *grad_scale : 1.f;            // as in k_adamw: unscale and clip in flight
    if (clip != nullptr) gs *= clip[2];
    const long base = ((long)blockIdx.x - j.cstart) * CHUNK;
    if (j.p_dtype == YOLO_F32 && j.g_dtype == YOLO_F32 && (j.n & 3) == 0 &&
        ((reinterpret_cast<uintptr_t>(j.p) | reinterpret_cast<uintptr_t>(j.g) | reinterpret_cast<uintptr_t>(j.m) |
          reinterpret_cast<uintptr_t>(ema)) & 15) == 0) {
        for (long i = base + threadIdx.x * 4L; i < base + CHUNK && i < j.n; i += 256 * 4) {
            float4 p = *reinterpret_cast<float4*>((float*)j.p + i);
            const float4 g = *reinterpret_cast<const float4*>((const float*)j.g + i);
            float4 m = *reinterpret_cast<float4*>(j.m + i);
            float* pp = &p.x; const float* gp = &g.x; float* mp = &m.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) sgd_elem(pp[k], gp[k], gs, mp[k], lr, mu, wd, nesterov);
            *reinterpret_cast<float4*>((float*)j.p + i) = p;
            *reinterpret_cast<float4*>(j.m + i) = m;
            if (ema != nullptr) ema_packet(ema, i, pp, df, omd);
        }
        return;
    }
    for (long i = base + threadIdx.x; i < base + CHUNK && i < j.n; i += 256) {
        float pv = ld_any(j.p, j.p_dtype, i), m = j.m[i];
        sgd_elem(pv, ld_any(j.g, j.g_dtype, i), gs, m, lr, mu, wd, nesterov);
        j.m[i] = m;
        st_any(j.p, j.p_dtype, i, pv);
        if (ema != nullptr) ema[i] = ema_elem(ema[i], as_stored(pv, j.p_dtype), df, omd);
    }
}

// e = d*e + (1-d)*p over a job table whose records carry p (read only) and e, g / m / v null: the tensors the optimizer
// does not step.  Launched after the AdamW launches of the step, so `updates` already counts this step; skip_flag non-zero
// (the step was skipped on overflow) leaves every shadow as it is.
__global__ __launch_bounds__(256) void k_ema_lerp(const AdamJob* __restrict__ jobs, int njobs, const double* __restrict__ ectl,
                                                  const float* __restrict__ skip_flag) {
    if (skip_flag != nullptr && *skip_flag != 0.f) return;
    __shared__ int sj;
    __shared__ float sc[2];
    if (threadIdx.x == 0) {
        sj = job_of_block(jobs, njobs);
        ema_coef(ectl, sc[0], sc[1]);
    }
    __syncthreads();
    const AdamJob j = jobs[sj];
    const float df = sc[0], omd = sc[1];
    if (j.e == nullptr) return;
    const long base = ((long)blockIdx.x - j.cstart) * CHUNK;
    for (long i = base + threadIdx.x; i < base + CHUNK && i < j.n; i += 256)
        j.e[i] = ema_elem(j.e[i], ld_any(j.p, j.p_dtype, i), df, omd);
}

// ---- global gradient norm (torch.nn.utils.clip_grad_norm_, norm_type 2; the reference's config.yaml carries
// training.grad_clip but its loop never reads it).  Same grid as k_adamw: one workgroup per 4096-element chunk writes
// ONE partial sum of squares with a plain store -- no float atomics, a replay gives the same bits.
// Accumulation depth: a lane owns 16 elements in four accumulators (4 fused multiply-adds each, the square itself is
// not rounded), 2 additions join the four, 6 shuffle steps join the wave, 2 additions join the four waves: at most
// 14 fp32 roundings on any path into a partial, all of non-negative terms, so a partial is within 14 * 2^-24 of its
// exact value (relative) -- inside the 32 roundings the tests' 2e-6 bound on the norm allows.
// With found_inf given, the pass also raises it on inf / nan and so replaces k_found_inf on the fp16 route.
__global__ __launch_bounds__(256) void k_grad_sqnorm(const AdamJob* __restrict__ jobs, int njobs, float* __restrict__ partials,
                                                     float* __restrict__ found_inf) {
    __shared__ int sj;
    __shared__ float sw[4];
    if (threadIdx.x == 0) {
        sj = job_of_block(jobs, njobs);
    }
    __syncthreads();
    const AdamJob j = jobs[sj];
    const long base = ((long)blockIdx.x - j.cstart) * CHUNK;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    bool bad = false;
    if (j.g_dtype == YOLO_F32 && (j.n & 3) == 0 && (reinterpret_cast<uintptr_t>(j.g) & 15) == 0) {
        for (long i = base + threadIdx.x * 4L; i < base + CHUNK && i < j.n; i += 256 * 4) {
            const float4 g = *reinterpret_cast<const float4*>((const float*)j.g + i);
            const float* gp = &g.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[k] = __fmaf_rn(gp[k], gp[k], acc[k]);
                bad |= !(fabsf(gp[k]) <= 3.4028234664e38f);     // inf or nan
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < CHUNK / 256; ++it) {
            const long i = base + threadIdx.x + it * 256L;
            if (i < j.n) {
                const float g = ld_any(j.g, j.g_dtype, i);
                acc[it & 3] = __fmaf_rn(g, g, acc[it & 3]);
                bad |= !(fabsf(g) <= 3.4028234664e38f);
            }
        }
    }
    if (found_inf != nullptr && bad) *found_inf = 1.f;        // every writer stores the same value
    const float w = wave_sum(__fadd_rn(__fadd_rn(acc[0], acc[1]), __fadd_rn(acc[2], acc[3])));
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = __fadd_rn(__fadd_rn(sw[0], sw[1]), __fadd_rn(sw[2], sw[3]));
}

// One workgroup: the partials summed in a fixed order in double (lane t takes t, t + 256, ...; then a fixed tree), so the
// result does not depend on scheduling.  state = fp32 [max_norm (read), total_norm, coef (written)];
// coef = min(1, max_norm / (total_norm + 1e-6)) like clip_grad_norm_ (an infinite norm gives 0, nan gives nan).
// grad_scale (GradScaler protocol or null): the norm is that of the unscaled gradients.
__global__ __launch_bounds__(256) void k_clip_finalize(const float* __restrict__ partials, long nparts, float* __restrict__ state,
                                                       const float* __restrict__ grad_scale) {
    __shared__ double sd[256];
    double s = 0.0;
    for (long i = threadIdx.x; i < nparts; i += 256) s += (double)partials[i];
    sd[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sd[threadIdx.x] += sd[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double inv = grad_scale ? 1.0 / (double)*grad_scale : 1.0;
        const double norm = sqrt(sd[0]) * inv;
        const double c = (double)state[0] / (norm + 1e-6);
        state[1] = (float)norm;
        state[2] = (float)(c < 1.0 ? c : (c != c ? c : 1.0));
    }
}

// ---- fp16 loss scaling on the device (torch.amp.GradScaler's protocol, reference src/training/train_model.py:195-208,
// 247-253, without its host round trips): found_inf over every gradient of the job table, then the optimizer kernel above
// (which skips on found_inf and unscales in flight), then the scale update -- all launches of a captured step.
__global__ __launch_bounds__(256) void k_found_inf(const AdamJob* __restrict__ jobs, int njobs, float* __restrict__ found_inf) {
    __shared__ int sj;
    if (threadIdx.x == 0) {
        sj = job_of_block(jobs, njobs);
    }
    __syncthreads();
    const AdamJob j = jobs[sj];
    const long base = ((long)blockIdx.x - j.cstart) * CHUNK;
    bool bad = false;
    for (long i = base + threadIdx.x; i < base + CHUNK && i < j.n; i += 256) {
        const float g = ld_any(j.g, j.g_dtype, i);
        bad |= !(fabsf(g) <= 3.4028234664e38f);             // inf or nan
    }
    if (bad) *found_inf = 1.f;                                // every writer stores the same value
}

// state = [scale, found_inf, last_found_inf] (fp32), tracker = successful steps since the last change.
// torch's _amp_update_scale_: overflow -> scale *= backoff, tracker = 0; else tracker + 1 == interval -> scale *= growth
// (if still finite), tracker = 0; else tracker += 1.  found_inf is handed on as last_found_inf and cleared for the next step.
__global__ void k_amp_update(float* __restrict__ state, int* __restrict__ tracker, float growth, float backoff, int interval) {
    const float found = state[1];
    if (found != 0.f) {
        state[0] *= backoff;
        *tracker = 0;
    } else {
        const int ok = *tracker + 1;
        if (ok == interval) {
            const float ns = state[0] * growth;
            if (fabsf(ns) <= 3.4028234664e38f) state[0] = ns;
            *tracker = 0;
        } else {
            *tracker = ok;
        }
    }
    state[2] = found;
    state[1] = 0.f;
}

}  // namespace

extern "C" {

int yolo_adamw_job_bytes(void) { return (int)sizeof(AdamJob); }

// write record `index` of the host-side table
int yolo_adamw_job_fill(void* jobs_host, int index, void* p, int p_dtype, const void* g, int g_dtype, float* m, float* v,
                        long n) {
    if (n < 0) return YOLO_ERR_ARG;
    AdamJob& j = ((AdamJob*)jobs_host)[index];
    j.p = p; j.g = g; j.m = m; j.v = v; j.n = n; j.cstart = 0; j.p_dtype = p_dtype; j.g_dtype = g_dtype;
    j.e = nullptr; j.ectl = nullptr;
    return YOLO_OK;
}

// the EMA shadow and control block of record `index` (after yolo_adamw_job_fill, which clears both); null = no EMA
int yolo_adamw_job_set_ema(void* jobs_host, int index, float* ema, double* ema_ctl) {
    if (index < 0) return YOLO_ERR_ARG;
    AdamJob& j = ((AdamJob*)jobs_host)[index];
    j.e = ema; j.ectl = ema_ctl;
    return YOLO_OK;
}

// only the gradient pointers of the n records changed (an eager loop's zero_grad(set_to_none=True) hands autograd fresh
// gradient tensors every step): one call instead of n yolo_adamw_job_fill calls
int yolo_adamw_jobs_set_grads(void* jobs_host, int njobs, const void* const* grads) {
    AdamJob* jobs = (AdamJob*)jobs_host;
    for (int i = 0; i < njobs; ++i) jobs[i].g = grads[i];
    return YOLO_OK;
}

// assign the chunk ranges; returns the number of workgroups
long yolo_adamw_jobs_finalize(void* jobs_host, int njobs) {
    AdamJob* jobs = (AdamJob*)jobs_host;
    long c = 0;
    for (int i = 0; i < njobs; ++i) {
        jobs[i].cstart = c;
        long nch = (jobs[i].n + CHUNK - 1) / CHUNK;
        c += nch > 0 ? nch : 1;
    }
    return c;
}

int yolo_adamw_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, const float* grad_scale,
                    const float* found_inf, hipStream_t st) {
    if (njobs <= 0 || nchunks <= 0) return YOLO_OK;
    hipLaunchKernelGGL(k_adamw_tick, dim3(1), dim3(1), 0, st, step, found_inf, (const AdamJob*)jobs_dev);
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, hyper, step,
                       grad_scale, found_inf, (const float*)nullptr);
    return YOLO_LAUNCH_CHECK();
}

// One optimizer step under dynamic loss scaling, all on the device: amp_state = [scale, found_inf (0 on entry), last_found_inf].
// The gradients of the job table carry the factor `scale` (the loss kernel multiplied its gradient by it in fp32).
int yolo_adamw_amp_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, float* amp_state,
                        int* growth_tracker, float growth_factor, float backoff_factor, int growth_interval, hipStream_t st) {
    if (njobs <= 0 || nchunks <= 0) return YOLO_OK;
    if (!(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f) || growth_interval < 1) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_found_inf, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, amp_state + 1);
    hipLaunchKernelGGL(k_adamw_tick, dim3(1), dim3(1), 0, st, step, amp_state + 1, (const AdamJob*)jobs_dev);
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, hyper, step,
                       amp_state, amp_state + 1, (const float*)nullptr);
    hipLaunchKernelGGL(k_amp_update, dim3(1), dim3(1), 0, st, amp_state, growth_tracker, growth_factor, backoff_factor, growth_interval);
    return YOLO_LAUNCH_CHECK();
}

// ---- clipped step.  Per step: yolo_grad_sqnorm for every job table (each into its own range of ONE partials buffer),
// one yolo_grad_clip_finalize over the whole buffer, then yolo_adamw_clip_step per table; under device loss scaling the
// norm pass raises found_inf = amp_state + 1 itself and yolo_amp_update_scale closes the step.
int yolo_grad_sqnorm(const void* jobs_dev, int njobs, long nchunks, float* partials, float* found_inf, hipStream_t st) {
    if (njobs <= 0 || nchunks <= 0) return YOLO_OK;
    if (partials == nullptr) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_grad_sqnorm, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, partials,
                       found_inf);
    return YOLO_LAUNCH_CHECK();
}

int yolo_grad_clip_finalize(const float* partials, long nparts, float* clip_state, const float* grad_scale, hipStream_t st) {
    if (partials == nullptr || clip_state == nullptr || nparts < 0) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_clip_finalize, dim3(1), dim3(256), 0, st, partials, nparts, clip_state, grad_scale);
    return YOLO_LAUNCH_CHECK();
}

int yolo_adamw_clip_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, const float* grad_scale,
                         const float* found_inf, const float* clip_state, hipStream_t st) {
    if (njobs <= 0 || nchunks <= 0) return YOLO_OK;
    if (clip_state == nullptr) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_adamw_tick, dim3(1), dim3(1), 0, st, step, found_inf, (const AdamJob*)jobs_dev);
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, hyper, step,
                       grad_scale, found_inf, clip_state);
    return YOLO_LAUNCH_CHECK();
}

int yolo_amp_update_scale(float* amp_state, int* growth_tracker, float growth_factor, float backoff_factor, int growth_interval,
                          hipStream_t st) {
    if (!(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f) || growth_interval < 1) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_amp_update, dim3(1), dim3(1), 0, st, amp_state, growth_tracker, growth_factor, backoff_factor, growth_interval);
    return YOLO_LAUNCH_CHECK();
}

// ---- SGD (k_sgd) on the machinery above: the job table with v null, k_adamw_tick, the norm pass, the scale update.
// clip_state null = unclipped; grad_scale / found_inf null = no loss scaling.
int yolo_sgd_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, const float* grad_scale,
                  const float* found_inf, const float* clip_state, hipStream_t st) {
    if (njobs <= 0 || nchunks <= 0) return YOLO_OK;
    hipLaunchKernelGGL(k_adamw_tick, dim3(1), dim3(1), 0, st, step, found_inf, (const AdamJob*)jobs_dev);
    hipLaunchKernelGGL(k_sgd, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, hyper, step, grad_scale,
                       found_inf, clip_state);
    return YOLO_LAUNCH_CHECK();
}

// yolo_adamw_amp_step's sequence around k_sgd: found_inf pass, tick, update, scale update
int yolo_sgd_amp_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, float* amp_state,
                      int* growth_tracker, float growth_factor, float backoff_factor, int growth_interval, hipStream_t st) {
    if (njobs <= 0 || nchunks <= 0) return YOLO_OK;
    if (!(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f) || growth_interval < 1) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_found_inf, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, amp_state + 1);
    hipLaunchKernelGGL(k_adamw_tick, dim3(1), dim3(1), 0, st, step, amp_state + 1, (const AdamJob*)jobs_dev);
    hipLaunchKernelGGL(k_sgd, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, hyper, step, amp_state,
                       amp_state + 1, (const float*)nullptr);
    hipLaunchKernelGGL(k_amp_update, dim3(1), dim3(1), 0, st, amp_state, growth_tracker, growth_factor, backoff_factor, growth_interval);
    return YOLO_LAUNCH_CHECK();
}

// EMA of the tensors the optimizer does not step (BatchNorm running statistics): records with p and e (g / m / v null), the
// chunk grid of the AdamW launches, d from ema_ctl as in k_adamw; nothing moves when *skip_flag != 0.
int yolo_ema_lerp(const void* jobs_dev, int njobs, long nchunks, const double* ema_ctl, const float* skip_flag, hipStream_t st) {
    if (njobs <= 0 || nchunks <= 0) return YOLO_OK;
    if (ema_ctl == nullptr) return YOLO_ERR_ARG;
    hipLaunchKernelGGL(k_ema_lerp, dim3((unsigned)nchunks), dim3(256), 0, st, (const AdamJob*)jobs_dev, njobs, ema_ctl, skip_flag);
    return YOLO_LAUNCH_CHECK();
}

}  // extern "C"
