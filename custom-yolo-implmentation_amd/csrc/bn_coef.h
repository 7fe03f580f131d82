// BatchNorm pieces shared by the kernels of elementwise.hip and the stem's one-pass backward (stem.hip): the activation
// gradient, the parameter accessors and the backward coefficients, each written once.
#pragma once
#include "common.h"

// sigmoid for the BatchNorm + SiLU kernels: hardware reciprocal (1 ulp) instead of the IEEE division -- the division
// expands to ~10 VALU instructions per element (v_div_scale x2, v_rcp, 4 fma, v_div_fmas, v_div_fixup) and these kernels
// are co-limited by VALU issue (a wave64 op takes 4 cycles on the 16-lane SIMD): about a quarter of their instructions
__device__ __forceinline__ float sigmoid_rcp(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

__device__ __forceinline__ float act_grad(float z, int act) {
    if (act == 0) return 1.f;
    float s = sigmoid_rcp(z);
    return s * (1.f + z * (1.f - s));
}

// BatchNorm parameters (gamma, beta -> dgamma, dbeta) and buffers (running statistics) in their own element type:
// fp32 under DDP / autocast, the low-precision parameter dtype under FSDP mixed precision, whose policy casts
// parameters AND buffers (reference src/training/utils_train.py:84-89,146-153).  Read / written once per channel in
// the prologues, arithmetic in fp32 / double as before, one rounding on the way out.
struct PIn {
    const void* p; int dt;
    __device__ __forceinline__ float ld(int i) const {
        return dt == YOLO_F32 ? ((const float*)p)[i] : dt == YOLO_BF16 ? (float)((const bf16_t*)p)[i] : (float)((const f16_t*)p)[i];
    }
};
struct PIo {
    void* p; int dt;
    __device__ __forceinline__ float ld(int i) const {
        return dt == YOLO_F32 ? ((const float*)p)[i] : dt == YOLO_BF16 ? (float)((const bf16_t*)p)[i] : (float)((const f16_t*)p)[i];
    }
    __device__ __forceinline__ void st(int i, float v) const {
        if (dt == YOLO_F32) ((float*)p)[i] = v; else if (dt == YOLO_BF16) ((bf16_t*)p)[i] = (bf16_t)v; else ((f16_t*)p)[i] = (f16_t)v;
    }
};
static inline bool pdt_ok(int dt) { return dt == YOLO_F32 || dt == YOLO_BF16 || dt == YOLO_F16; }

// Backward: (sum dz, sum dz*y) in double -> dbeta = sum dz, dgamma = sum dz*yhat = invstd*(sum dz*y - mean*sum dz), and
// dy = k0*(dz - c1 - yhat*c2), yhat = (y-mean)*invstd  ==  A*dz + B*y + D  (three constants per channel).
// The double form is what the stem's finalize multiplies its three pixel sums with (B*G2 + D*G3 cancel when |mean| / std
// is large); the fp32 form, its rounding, is what the apply kernels keep per channel.
struct BnBwdCoefD { double dbeta, dgamma, A, B, D; };
__device__ __forceinline__ BnBwdCoefD bn_bwd_coef_d(double s, double q, float count, const PIn& gamma, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, int c) {
    const double is = invstd[c], mu = mean[c];
    q = is * (q - mu * s);
    const double k0 = (double)gamma.ld(c) * is, c1 = s / count, c2 = q / count;
    BnBwdCoefD k;
    k.dbeta = s;
    k.dgamma = q;
    k.A = k0;
    k.B = -k0 * c2 * is;
    k.D = -k0 * c1 + k0 * c2 * mu * is;
    return k;
}
struct BnBwdCoef { float dbeta, dgamma, A, B, D; };
__device__ __forceinline__ BnBwdCoef bn_bwd_coef(double s, double q, float count, const PIn& gamma, const float* __restrict__ mean,
                                                 const float* __restrict__ invstd, int c) {
    const BnBwdCoefD d = bn_bwd_coef_d(s, q, count, gamma, mean, invstd, c);
    BnBwdCoef k;
    k.dbeta = (float)d.dbeta;
    k.dgamma = (float)d.dgamma;
    k.A = (float)d.A;
    k.B = (float)d.B;
    k.D = (float)d.D;
    return k;
}
