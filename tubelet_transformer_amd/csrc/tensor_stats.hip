// Per-tensor gradient / parameter / update statistics of the flat fp32 buffers as one segmented streaming reduction behind the AdamW
// launches (gfx950): the step monitor (monitor.py).  One 8-float row per parameter tensor:
//   0 sum g^2 (finite g)   1 max |g| (finite g)   2 number of non-finite g   3 number of g == +-0
//   4 sum p^2 (finite p)   5 max |p| (finite p)   6 number of non-finite p   7 sum u^2, u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps)
// u is the AdamW direction of adamw_kernel (optim.hip) before lr and without the decay term.  The reference has no counterpart: it logs the
// loss terms only (utils/video_action_recognition.py:182-220).  Deterministic and atomic-free, three launches:
//   1. tensor_stats_chunk_kernel   a workgroup of 256 threads reduces one chunk (<= TSTATS_CHUNK elements of ONE tensor) to 8 partials
//   2. tensor_stats_rows_kernel    a wave per tensor reduces its chunk partials in a fixed order and writes the row
//   3. tensor_stats_count_kernel   one thread advances the counters, so every thread of 1. and 2. read the same values
// Whether a launch records, and where the row goes (a ring slot, or the keep-first slot of a step the optimizer skipped), is decided ON THE
// DEVICE from the AdamW step count, the clip coefficient and a small state block: a replayed hipGraph records at the cadence the state
// holds.  HBM-bound: 4 streams of 4 B per element, read only.
#include "common.h"

#define TSTATS_CHUNK 8192         // elements per chunk: 256 threads x 8 float4; a multiple of 64, so every chunk starts 16-byte aligned
#define TSTATS_MAX_BLOCKS 2048    // 256 CUs x 8 workgroups of 256 threads; more chunks than that are walked with a grid stride
#define TSTATS_COUNT_MAX 16777216.f   // counts travel as floats: exact below 2^24, saturated there

// state (4 x 32 bit, device): {every, history, bad_count, bad_step}
#define TSTATS_EVERY 0
#define TSTATS_HISTORY 1
#define TSTATS_BAD_COUNT 2
#define TSTATS_BAD_STEP 3

struct TensorStatsTensor {        // one parameter tensor (tuber_tensor_stats_tensor_bytes)
    int chunk0, nchunks;          // its chunks: [chunk0, chunk0 + nchunks) of the chunk table, ascending offsets; together they hold its numel
    float beta1, beta2, eps;      // of its parameter group (zeros: in no group)
};
struct TensorStatsChunk {         // a run of <= TSTATS_CHUNK elements of one tensor (tuber_tensor_stats_chunk_bytes)
    long off;                     // first element in the flat buffers (the tensor's 64-element aligned window start + a multiple of the chunk)
    int n;                        // elements
    int tensor;                   // row of the tensor table
};

// where does this launch's table go?  -1: nowhere (every workgroup returns at once); [0, history): that ring slot; history: the bad slot
// (a step AdamW skipped: clip[1] < 0 -- kept only while bad_count == 0).  *t = the AdamW step count (0 without step_ptr).
__device__ __forceinline__ int tstats_slot(const int* __restrict__ state, int history, const int* __restrict__ step_ptr,
                                           const float* __restrict__ clip, int* t) {
    *t = step_ptr ? *step_ptr : 0;
    if (clip && clip[1] < 0.f) return state[TSTATS_BAD_COUNT] == 0 ? history : -1;
    if (!step_ptr) return 0;
    const int every = state[TSTATS_EVERY] > 0 ? state[TSTATS_EVERY] : 1;
    if (*t % every != 0) return -1;
    return (*t / every) % history;
}

__device__ __forceinline__ bool tstats_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// 1 - beta^t in fp64 from the fp32 beta (square and multiply, t >= 1), for the caller to round once; 1 for t < 1 (no step taken yet)
__device__ __forceinline__ double tstats_bias_correction(float beta, int t) {
    if (t < 1) return 1.0;
    double b = (double)beta, r = 1.0;
    for (unsigned e = (unsigned)t; e; e >>= 1) {
        if (e & 1) r *= b;
        b *= b;
    }
    return 1.0 - r;
}

struct TStatsAcc {
    float gss, gmax, gnf, gz, pss, pmax, pnf, uss;
};

__device__ __forceinline__ void tstats_gp(TStatsAcc& a, float g, float p) {
    const bool gf = tstats_finite(g), pf = tstats_finite(p);
    const float ga = gf ? fabsf(g) : 0.f, pa = pf ? fabsf(p) : 0.f;
    a.gss += ga * ga; a.gmax = fmaxf(a.gmax, ga); a.gnf += gf ? 0.f : 1.f; a.gz += g == 0.f ? 1.f : 0.f;
    a.pss += pa * pa; a.pmax = fmaxf(a.pmax, pa); a.pnf += pf ? 0.f : 1.f;
}

__device__ __forceinline__ void tstats_u(TStatsAcc& a, float m, float v, float bc1, float bc2s, float eps) {
    const float u = m == 0.f ? 0.f : (m / bc1) / (sqrtf(v) / bc2s + eps);      // (m == 0: a tensor no group updates has eps = 0 too)
    a.uss += u * u;
}

__global__ __launch_bounds__(256) void tensor_stats_chunk_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                                 const float* __restrict__ m, const float* __restrict__ v,
                                                                 const TensorStatsTensor* __restrict__ tensors,
                                                                 const TensorStatsChunk* __restrict__ chunks, int n_chunks,
                                                                 float* __restrict__ partial, const int* __restrict__ state, int history,
                                                                 const int* __restrict__ step_ptr, const float* __restrict__ clip) {
    __shared__ float red[8][4];
    int t;
    if (tstats_slot(state, history, step_ptr, clip, &t) < 0) return;
    const bool moments = m && v;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const TensorStatsChunk ch = chunks[c];
        const TensorStatsTensor te = tensors[ch.tensor];
        const float bc1 = (float)tstats_bias_correction(te.beta1, t), bc2s = (float)sqrt(tstats_bias_correction(te.beta2, t));
        const float4* g4 = (const float4*)(g + ch.off);
        const float4* p4 = (const float4*)(p + ch.off);
        TStatsAcc a = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int n4 = ch.n >> 2;
#pragma unroll 2
        for (int i = threadIdx.x; i < n4; i += 256) {
            const float4 gv = g4[i], pv = p4[i];
            tstats_gp(a, gv.x, pv.x); tstats_gp(a, gv.y, pv.y); tstats_gp(a, gv.z, pv.z); tstats_gp(a, gv.w, pv.w);
            if (moments) {
                const float4 mv = ((const float4*)(m + ch.off))[i], vv = ((const float4*)(v + ch.off))[i];
                tstats_u(a, mv.x, vv.x, bc1, bc2s, te.eps); tstats_u(a, mv.y, vv.y, bc1, bc2s, te.eps);
                tstats_u(a, mv.z, vv.z, bc1, bc2s, te.eps); tstats_u(a, mv.w, vv.w, bc1, bc2s, te.eps);
            }
        }
        const int i = (n4 << 2) + threadIdx.x;           // the tensor's tail: at most 3 elements
        if (i < ch.n) {
            tstats_gp(a, g[ch.off + i], p[ch.off + i]);
            if (moments) tstats_u(a, m[ch.off + i], v[ch.off + i], bc1, bc2s, te.eps);
        }
        const float w[8] = {wave_sum(a.gss), wave_max(a.gmax), wave_sum(a.gnf), wave_sum(a.gz),
                            wave_sum(a.pss), wave_max(a.pmax), wave_sum(a.pnf), wave_sum(a.uss)};
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[j][threadIdx.x >> 6] = w[j];
        }
        __syncthreads();
        if (threadIdx.x < 8) {
            const float* r = red[threadIdx.x];
            const bool is_max = threadIdx.x == 1 || threadIdx.x == 5;
            partial[(long)c * 8 + threadIdx.x] = is_max ? fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])) : r[0] + r[1] + r[2] + r[3];
        }
        __syncthreads();
    }
}

// one wave per tensor: lane = 8 * group + column; group j adds the chunks j, j + 8, ... in ascending order, then the 8 groups meet in a
// fixed exchange tree (the same value in every lane: fp32 addition commutes)
__global__ __launch_bounds__(256) void tensor_stats_rows_kernel(const TensorStatsTensor* __restrict__ tensors, int n_tensors,
                                                                const float* __restrict__ partial, const int* __restrict__ state,
                                                                int history, float* __restrict__ ring, float* __restrict__ bad,
                                                                const int* __restrict__ step_ptr, const float* __restrict__ clip) {
    int t;
    const int slot = tstats_slot(state, history, step_ptr, clip, &t);
    if (slot < 0) return;
    const int ti = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ti >= n_tensors) return;
    const int lane = threadIdx.x & 63, col = lane & 7, grp = lane >> 3;
    const bool is_max = col == 1 || col == 5, is_count = col == 2 || col == 3 || col == 6;
    const TensorStatsTensor te = tensors[ti];
    float acc = 0.f;
    for (int c = grp; c < te.nchunks; c += 8) {
        const float x = partial[(long)(te.chunk0 + c) * 8 + col];
        acc = is_max ? fmaxf(acc, x) : acc + x;
        if (is_count) acc = fminf(acc, TSTATS_COUNT_MAX);
    }
#pragma unroll
    for (int s = 8; s < 64; s <<= 1) {
        const float x = __shfl_xor(acc, s, 64);
        acc = is_max ? fmaxf(acc, x) : acc + x;
        if (is_count) acc = fminf(acc, TSTATS_COUNT_MAX);
    }
    float* dst = slot == history ? bad : ring + (long)slot * n_tensors * 8;
    if (grp == 0) dst[(long)ti * 8 + col] = acc;
}

// the bookkeeping of the row just written, in a launch of its own: every thread of the two launches before it read the same state
__global__ void tensor_stats_count_kernel(int* __restrict__ state, int history, int* __restrict__ row_step, float* __restrict__ row_norm,
                                          const int* __restrict__ step_ptr, const float* __restrict__ clip) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int t;
    const int slot = tstats_slot(state, history, step_ptr, clip, &t);
    if (clip && clip[1] < 0.f) {
        if (state[TSTATS_BAD_COUNT] == 0) state[TSTATS_BAD_STEP] = t;
        if (state[TSTATS_BAD_COUNT] < 0x7fffffff) state[TSTATS_BAD_COUNT] += 1;
    } else if (slot >= 0) {
        row_step[slot] = t;
        row_norm[2 * slot] = clip ? clip[0] : 0.f;
        row_norm[2 * slot + 1] = clip ? clip[1] : 1.f;
    }
}

extern "C" {

// Statistics of n_tensors parameter tensors over the flat buffers g (gradient), p (parameters), m / v (the Adam moments; either NULL: column 7
// is 0), all 16-byte aligned.  tensors / chunks: DEVICE tables of TensorStatsTensor / TensorStatsChunk; partial: n_chunks x 8 floats of
// scratch.  state: DEVICE int[4] {every, history, bad_count, bad_step}.  With step_ptr (the AdamW step count t, already advanced on a good
// step) and clip (norm_out of tuber_grad_norm_clip_coef): a good step records iff t % every == 0, into ring[(t / every) % history]
// ([history][n_tensors][8]) with row_step[slot] = t and row_norm[slot] = {clip[0], clip[1]}; a skipped step (clip[1] < 0) writes bad
// ([n_tensors][8]) and bad_step = t only while bad_count == 0, and always advances bad_count.  A NULL clip counts as a good step; a NULL
// step_ptr drops the cadence (ring slot 0, row_step 0, no bias correction).
int tuber_tensor_stats(const float* g, const float* p, const float* m, const float* v, const void* tensors, int n_tensors,
                       const void* chunks, int n_chunks, float* partial, int* state, int history, int* row_step, float* row_norm,
                       float* ring, float* bad, const int* step_ptr, const float* clip, hipStream_t stream) {
    if (!g || !p || !tensors || !chunks || !partial || !state || !row_step || !row_norm || !ring || !bad) return TUBER_EINVAL;
    if (n_tensors <= 0 || n_chunks <= 0 || history < 1) return TUBER_EINVAL;
    if ((((uintptr_t)g) | ((uintptr_t)p) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) return TUBER_EINVAL;
    const int nb = n_chunks < TSTATS_MAX_BLOCKS ? n_chunks : TSTATS_MAX_BLOCKS;
    hipLaunchKernelGGL(tensor_stats_chunk_kernel, dim3(nb), dim3(256), 0, stream, g, p, m, v, (const TensorStatsTensor*)tensors,
                       (const TensorStatsChunk*)chunks, n_chunks, partial, state, history, step_ptr, clip);
    hipLaunchKernelGGL(tensor_stats_rows_kernel, dim3((n_tensors + 3) / 4), dim3(256), 0, stream, (const TensorStatsTensor*)tensors, n_tensors,
                       partial, state, history, ring, bad, step_ptr, clip);
    hipLaunchKernelGGL(tensor_stats_count_kernel, dim3(1), dim3(64), 0, stream, state, history, row_step, row_norm, step_ptr, clip);
    TUBER_RETURN_LAUNCH();
}
int tuber_tensor_stats_chunk() { return TSTATS_CHUNK; }
int tuber_tensor_stats_tensor_bytes() { return (int)sizeof(TensorStatsTensor); }
int tuber_tensor_stats_chunk_bytes() { return (int)sizeof(TensorStatsChunk); }

}  // extern "C"
