// Weight averaging (EMA / SWA) of the flat fp32 parameter buffer as one streaming pass behind the AdamW launches (gfx950).
// Restates timm's ModelEmaV2 (ema = decay * ema + (1 - decay) * p, with the optional warm-up ramp min(decay, (1 + n) / (10 + n))) and the
// default avg_fn of torch.optim.swa_utils.AveragedModel (avg += (p - avg) / n) in the lerp form avg += w * (p - avg): an element with
// p == avg keeps its bits for ever (frozen parameters, the padding between the 64-element slots).  The weight w, the cadence and the skip of
// a non-finite step are decided ON THE DEVICE from device memory, so a replayed hipGraph averages with the right weight every step and a
// changed decay needs no new capture.  HBM-bound: 3 streams of 4 B per element (read p, read avg, write avg).
#include "common.h"

// table (5 x 32 bit, device): {decay (float bits), mode (0 ema, 1 swa), warmup (0 / 1), start, period}
#define WAVG_DECAY 0
#define WAVG_MODE 1
#define WAVG_WARMUP 2
#define WAVG_START 3
#define WAVG_PERIOD 4

// does this launch average?  clip = norm_out of tuber_grad_norm_clip_coef: clip[1] < 0 is the step AdamW skipped.  step_ptr = the AdamW step
// count t (already advanced by this step): the update happens iff t >= start and (t - start) % period == 0.  A NULL pointer drops its test.
__device__ __forceinline__ bool wavg_applies(const int* __restrict__ table, const int* __restrict__ step_ptr, const float* __restrict__ clip) {
    if (clip && clip[1] < 0.f) return false;
    if (step_ptr) {
        const int t = *step_ptr, start = table[WAVG_START];
        const int period = table[WAVG_PERIOD] > 0 ? table[WAVG_PERIOD] : 1;
        if (t < start || (t - start) % period != 0) return false;
    }
    return true;
}

// the weight of update number n (counted from 1), formed in fp64 from the fp32 decay and rounded once -- weight_avg.effective_weight on the host
__device__ __forceinline__ float wavg_weight(const int* __restrict__ table, int n) {
    if (table[WAVG_MODE] == 1) return (float)(1.0 / (double)n);
    double d = (double)__int_as_float(table[WAVG_DECAY]);
    if (table[WAVG_WARMUP]) {
        const double ramp = (1.0 + (double)n) / (10.0 + (double)n);
        if (ramp < d) d = ramp;
    }
    return (float)(1.0 - d);
}

__device__ __forceinline__ float wavg_one(float a, float p, float w) {
    return p == a ? a : a + w * (p - a);             // (the select keeps a -0.0 that a + w * 0 would turn into +0.0)
}

__global__ __launch_bounds__(256) void weight_average_kernel(float* __restrict__ avg, const float* __restrict__ p, long n,
                                                            const int* __restrict__ table, const int* __restrict__ n_avg,
                                                            const int* __restrict__ step_ptr, const float* __restrict__ clip) {
    if (!wavg_applies(table, step_ptr, clip)) return;
    const float w = wavg_weight(table, *n_avg + 1);
    const bool copy = w == 1.f;                      // first SWA update (and decay 0): avg = p exactly
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 pv = ((const float4*)p)[i];
        float4 av = ((const float4*)avg)[i];
        if (copy) {
            av = pv;
        } else {
            av.x = wavg_one(av.x, pv.x, w); av.y = wavg_one(av.y, pv.y, w);
            av.z = wavg_one(av.z, pv.z, w); av.w = wavg_one(av.w, pv.w, w);
        }
        ((float4*)avg)[i] = av;
    }
    if (blockIdx.x == 0)
        for (long i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x) avg[i] = copy ? p[i] : wavg_one(avg[i], p[i], w);
}

// n_avg += 1 iff the streaming launch before it averaged: a launch of its own, so that every thread of that launch read the same count
__global__ void weight_average_count_kernel(const int* __restrict__ table, int* __restrict__ n_avg, const int* __restrict__ step_ptr,
                                            const float* __restrict__ clip) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && wavg_applies(table, step_ptr, clip)) *n_avg += 1;
}

extern "C" {

#define WAVG_MAX_BLOCKS 2048      // 256 CUs x 8 workgroups of 256 threads; longer buffers grid-stride

// avg[i] += w * (p[i] - avg[i]) over [0, n); table = device {decay, mode, warmup, start, period}, n_avg = device update count (advanced by one
// iff the update was applied).  step_ptr / clip: the AdamW step count and norm_out of tuber_grad_norm_clip_coef (cadence and the skip of a
// non-finite step, both decided on the device), or NULL: unconditional.  avg and p 16-byte aligned.
int tuber_weight_average(float* avg, const float* p, long n, const int* table, int* n_avg, const int* step_ptr, const float* clip,
                         hipStream_t stream) {
    if (n <= 0 || !avg || !p || !table || !n_avg) return TUBER_EINVAL;
    if ((((uintptr_t)avg) | ((uintptr_t)p)) & 15) return TUBER_EINVAL;
    long nb = (n / 4 + 255) / 256;
    if (nb > WAVG_MAX_BLOCKS) nb = WAVG_MAX_BLOCKS;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(weight_average_kernel, dim3((int)nb), dim3(256), 0, stream, avg, p, n, table, n_avg, step_ptr, clip);
    hipLaunchKernelGGL(weight_average_count_kernel, dim3(1), dim3(64), 0, stream, table, n_avg, step_ptr, clip);
    TUBER_RETURN_LAUNCH();
}

}  // extern "C"
