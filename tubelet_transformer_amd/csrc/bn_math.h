// BatchNorm's per-channel arithmetic, defined ONCE: the kernels that finalise statistics or derive backward coefficients (norm.hip, the
// forward finalisation of dwconv_tile.hip) call these, so the paths that tests compare bit for bit share their expressions.  Plain values in,
// plain values out: callers keep their own loads, stores, guards and reductions.  `count` and `eps` stay float and are widened here.
// Every product that feeds a sum is an explicit fma / fmaf: left to -ffp-contract=fast, whether and which product is fused depends on the code
// around the inlined call, and these results are compared bit for bit across kernels.  (The forms are the ones the compiler chose when the
// expressions stood written out in the kernels.)
#pragma once
#include "common.h"

// acc[0..3] += v.{x, y, z, w}
__device__ __forceinline__ void add4(double (&acc)[4], const float4 v) { acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w; }
__device__ __forceinline__ void add4(float (&acc)[4], const float4 v) { acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w; }

// invstd of the train-mode finalisation: fp64, rounded once
__device__ __forceinline__ float bn_invstd(double var, float eps) { return (float)(1.0 / sqrt(var + (double)eps)); }

// forward finalisation from (sum x, sum x^2) over `count` elements: biased variance clamped at 0, scale = gamma * invstd, shift = beta - mean * scale
struct BnStats { double mean, var; float invstd, scale, shift; };
__device__ __forceinline__ BnStats bn_finalize(double sum_x, double sum_xx, float count, float eps, float gamma, float beta) {
    BnStats s;
    s.mean = sum_x / (double)count;
    s.var = fma(-s.mean, s.mean, sum_xx / (double)count);
    if (s.var < 0.0) s.var = 0.0;
    s.invstd = bn_invstd(s.var, eps);
    s.scale = gamma * s.invstd;
    s.shift = fmaf(-(float)s.mean, s.scale, beta);
    return s;
}

// running statistics after this batch: unbiased variance, blended with factor m = the module's momentum, or bn_cumulative_factor(n) for the
// cumulative average of momentum=None (n = num_batches_tracked BEFORE this batch; a function of its own so that the caller reads n only then)
__device__ __forceinline__ float bn_cumulative_factor(long long n) { return (float)(1.0 / (double)(n + 1)); }
struct BnRunning { float mean, var; };
__device__ __forceinline__ BnRunning bn_running_update(double mean, double var, float count, float m, float rmean0, float rvar0) {
    const double unbiased = count > 1.f ? var * (double)count / ((double)count - 1.0) : var;
    return {fmaf(m, (float)mean, (1.f - m) * rmean0), fmaf(m, (float)unbiased, (1.f - m) * rvar0)};
}

// the constant affine map of an eval-mode layer (fp32 throughout, as the eval path has always formed it)
struct BnAffine { float scale, shift; };
__device__ __forceinline__ BnAffine bn_eval_affine(float gamma, float beta, float rmean, float rvar, float eps) {
    const float sc = gamma / sqrtf(rvar + eps);
    return {sc, fmaf(-rmean, sc, beta)};
}

// backward from (sum dz, sum dz*x): dL/dx = cA*dz + cB*x + cC, dgamma += sum dz*xhat, dbeta += sum dz.
// FRZ: the frozen layer (module in eval mode) is a constant affine map: cA = gamma * invstd, cB = cC = 0, count is not used.
struct BnBwd { float cA, cB, cC, dgamma, dbeta; };
template <bool FRZ = false>
__device__ __forceinline__ BnBwd bn_bwd_coefs(double sum_dz, double sum_dz_x, float mean, float invstd, float gamma, float count) {
    const double mu = mean, r = invstd, g = gamma;
    const double sum_dz_xhat = fma(-mu, sum_dz, sum_dz_x) * r;
    BnBwd o;
    o.cA = (float)(g * r);
    if constexpr (FRZ) {
        o.cB = 0.f;
        o.cC = 0.f;
    } else {
        const double m1 = sum_dz / count, m2 = sum_dz_xhat / count;
        o.cB = (float)(-g * r * r * m2);
        o.cC = (float)fma(g * r * r * m2, mu, -(g * r * m1));
    }
    o.dgamma = (float)sum_dz_xhat;
    o.dbeta = (float)sum_dz;
    return o;
}
