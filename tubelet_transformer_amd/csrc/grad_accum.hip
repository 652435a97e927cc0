// Gradient accumulation over micro-batches (accum.py): one pass over the trainable windows of the flat fp32 gradient buffer, and the
// one-launch snapshot / restore of the BatchNorm running statistics that keeps micro-batches 1..m-1 from updating them.
#include "common.h"

namespace {

constexpr int ACC_THREADS = 256;
constexpr int ACC_BLOCKS_PER_CU = 4;

template <int MODE>
__device__ __forceinline__ void accum_one(float* __restrict__ g, float* __restrict__ acc, long i, float s) {
    if (MODE == 0) {
        acc[i] = g[i];
    } else if (MODE == 1) {
        acc[i] = acc[i] + g[i];
    } else {
        g[i] = (acc[i] + g[i]) * s;
    }
}

template <int MODE>
__device__ __forceinline__ void accum_vec(float4* __restrict__ g, float4* __restrict__ acc, long i, float s) {
    const float4 x = g[i];
    if (MODE == 0) {
        acc[i] = x;
    } else if (MODE == 1) {
        float4 a = acc[i];
        a.x = a.x + x.x; a.y = a.y + x.y; a.z = a.z + x.z; a.w = a.w + x.w;
        acc[i] = a;
    } else {
        const float4 a = acc[i];
        float4 y;
        y.x = (a.x + x.x) * s; y.y = (a.y + x.y) * s; y.z = (a.z + x.z) * s; y.w = (a.w + x.w) * s;
        g[i] = y;
    }
}

// every thread walks the window table; each window is spread over the whole grid: a scalar head up to the first 16-byte boundary,
// float4 body, scalar tail.  Windows are a few large ranges (trainable_ranges), so the per-window setup is negligible.
template <int MODE>
__global__ __launch_bounds__(ACC_THREADS) void grad_accum_kernel(float* __restrict__ g, float* __restrict__ acc,
                                                                 const long* __restrict__ win, int nwin,
                                                                 const float* __restrict__ scale_dev, float scale) {
    const float s = scale_dev ? scale_dev[0] : scale;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nthr = (long)gridDim.x * blockDim.x;
    for (int w = 0; w < nwin; ++w) {
        const long b = win[2 * w], e = win[2 * w + 1];
        if (e <= b) continue;
        long vb = (b + 3) & ~3L;                  // base pointers are 16-byte aligned (checked on the host): element 4k starts a float4
        if (vb > e) vb = e;
        const long nv = (e - vb) >> 2;
        const long ve = vb + 4 * nv;
        const long nhead = vb - b, ntail = e - ve;
        for (long j = tid; j < nhead + ntail; j += nthr)
            accum_one<MODE>(g, acc, j < nhead ? b + j : ve + (j - nhead), s);
        float4* g4 = reinterpret_cast<float4*>(g + vb);
        float4* a4 = reinterpret_cast<float4*>(acc + vb);
        for (long i = tid; i < nv; i += nthr) accum_vec<MODE>(g4, a4, i, s);
    }
}

// 32-bit words of BatchNorm buffers <-> one arena: row r = {buffer address, arena offset (words), words}
__global__ void bn_stats_copy_kernel(const long* __restrict__ table, unsigned* __restrict__ arena, int restore) {
    const long* row = table + 3 * blockIdx.y;
    unsigned* buf = reinterpret_cast<unsigned*>(row[0]);
    unsigned* a = arena + row[1];
    const long n = row[2];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (restore) buf[i] = a[i];
        else a[i] = buf[i];
    }
}

int cu_count() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;
        n = v;
    }
    return n;
}

}  // namespace

extern "C" {

// mode 0 (init): acc[w] = g[w]; 1 (add): acc[w] += g[w]; 2 (fold): g[w] = (acc[w] + g[w]) * scale, scale = scale_dev[0] when given.
// windows: DEVICE table of nwin int64 pairs [begin, end) in elements.  g and acc must be 16-byte aligned.
int tuber_grad_accum(float* g, float* acc, const long* windows, int nwin, int mode, const float* scale_dev, float scale, hipStream_t stream) {
    if (!g || !acc || !windows || nwin <= 0 || mode < 0 || mode > 2) return TUBER_EINVAL;
    if ((reinterpret_cast<unsigned long long>(g) | reinterpret_cast<unsigned long long>(acc)) & 15) return TUBER_EINVAL;
    const dim3 grid(cu_count() * ACC_BLOCKS_PER_CU), block(ACC_THREADS);
    if (mode == 0) hipLaunchKernelGGL(grad_accum_kernel<0>, grid, block, 0, stream, g, acc, windows, nwin, scale_dev, scale);
    else if (mode == 1) hipLaunchKernelGGL(grad_accum_kernel<1>, grid, block, 0, stream, g, acc, windows, nwin, scale_dev, scale);
    else hipLaunchKernelGGL(grad_accum_kernel<2>, grid, block, 0, stream, g, acc, windows, nwin, scale_dev, scale);
    TUBER_RETURN_LAUNCH();
}

// restore 0: arena <- buffers (snapshot); 1: buffers <- arena.  table: DEVICE [nrows][3] int64 rows {address, arena word offset, words};
// max_words: the largest row (grid width).
int tuber_bn_stats_copy(const long* table, int nrows, float* arena, long max_words, int restore, hipStream_t stream) {
    if (!table || !arena || nrows <= 0 || nrows > 65535 || max_words <= 0) return TUBER_EINVAL;
    long bx = (max_words + 255) / 256;
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(bn_stats_copy_kernel, dim3((int)bx, nrows), dim3(256), 0, stream, table, reinterpret_cast<unsigned*>(arena), restore);
    TUBER_RETURN_LAUNCH();
}

}  // extern "C"
