// Whole-video inference on gfx950: the overlapping clips of a batch of key frames gathered from ONE resident video (video.VideoDetector).
// The reference cuts a clip per key frame on CPU workers (datasets/ava_frame.py:43,143-150: every FRAME_RATE-th frame, the ends clamped;
// datasets/jhmdb_frame.py:201-213: the ends padded) and normalises it (datasets/video_transforms.py:308-322); here the frames sit in HBM once,
// at working resolution, and a clip is a row of a frame-index table:
//     out[b][c][t][y][x] = lut[c][frames[clamp(index[b][t], 0, nframes - 1)][y1 + y][x1 + x][c]]
// 3 B read and 12 B written per output pixel: the kernel is bound by its stores.  A thread owns 4 consecutive output pixels of one (b, t, y):
// three 16-byte stores, fed by the 12 source bytes taken as dwords from the enclosing 4-byte-aligned window (a frame row starts at any byte
// offset: W * 3 is rarely a multiple of 4) and shifted into place.  w % 4 != 0 (or an `out` that is not 16-byte aligned) takes byte loads
// and scalar stores.  The normalisation table (3 KB) is staged in LDS, as clip_prepare_kernel does.
// video.VideoStream keeps only a ring of the last R frames: video_clips_ring_kernel is the same gather with the frame picked by the index rule
// itself (video.clip_indices in closed form) and mapped to its ring slot; the load / store body is one function both kernels call.
#include "common.h"

namespace {

// The body both kernels share: the (up to) 4 output pixels at o, o + cstride, o + 2 * cstride from the 12 source bytes at p.  V4: w % 4 == 0 and
// out 16-byte aligned; [buf_lo, buf_hi): the bytes of the frame buffer that may be touched; left: pixels of the row from p on (scalar form).
template <bool V4>
__device__ __forceinline__ void video_clips_quad(const uint8_t* p, const uint8_t* buf_lo, const uint8_t* buf_hi, const float* s_lut, float* o,
                                                 long cstride, int left) {
    if (V4) {
        const int sh = (int)((uintptr_t)p & 3);
        const uint8_t* ap = p - sh;
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint8_t* g = ap + 4 * j;
            if (j == 3 && sh == 0) v[j] = 0;                           // the 12 bytes end with the third dword
            else if (g >= buf_lo && g + 4 <= buf_hi) v[j] = *(const uint32_t*)g;
            else {                                                     // the first / last dword of the buffer: its bytes one by one
                v[j] = 0;
                for (int e = 0; e < 4; ++e)
                    if (g + e >= buf_lo && g + e < buf_hi) v[j] |= (uint32_t)g[e] << (8 * e);
            }
        }
        uint32_t d[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) d[j] = (uint32_t)(((((unsigned long long)v[j + 1]) << 32) | v[j]) >> (8 * sh));
        float q[3][4];
#pragma unroll
        for (int k = 0; k < 12; ++k) q[k % 3][k / 3] = s_lut[(k % 3) * 256 + ((d[k >> 2] >> (8 * (k & 3))) & 255u)];
#pragma unroll
        for (int c = 0; c < 3; ++c) *(float4*)(o + c * cstride) = make_float4(q[c][0], q[c][1], q[c][2], q[c][3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= left) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c * cstride + j] = s_lut[c * 256 + p[3 * j + c]];
        }
    }
}

template <bool V4>
__global__ __launch_bounds__(256) void video_clips_kernel(const uint8_t* __restrict__ frames, int nframes, int H, int W,
                                                          const int* __restrict__ index, int B, int T, int y1, int x1, int h, int w,
                                                          const float* __restrict__ lut, float* __restrict__ out) {
    __shared__ float s_lut[3 * 256];
    for (int i = threadIdx.x; i < 768; i += blockDim.x) s_lut[i] = lut[i];
    __syncthreads();
    const uint8_t* buf_lo = frames;                                    // [buf_lo, buf_hi): the bytes of `frames` that may be touched
    const uint8_t* buf_hi = frames + (long)nframes * H * W * 3;
    const int quads = (w + 3) >> 2;
    const long total = (long)B * T * h * quads;
    const long plane = (long)h * w;
    const long cstride = (long)T * plane;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int xq = (int)(i % quads);
        long r = i / quads;
        const int y = (int)(r % h); r /= h;
        const int t = (int)(r % T), b = (int)(r / T);
        const int f = min(max(index[(long)b * T + t], 0), nframes - 1);            // clamped here: the table may hold anything
        const uint8_t* p = frames + ((((long)f * H + y1 + y) * W) + x1 + xq * 4) * 3;
        float* o = out + ((long)b * 3 * T + t) * plane + (long)y * w + xq * 4;
        video_clips_quad<V4>(p, buf_lo, buf_hi, s_lut, o, cstride, w - xq * 4);
    }
}

// The frame at position t of the clip around `key`: video.clip_indices' three rules in closed form.  n < 0: the video's end is not known (and,
// the caller guarantees, not needed: the row would be the same for every longer video); otherwise its frame count.
__device__ __forceinline__ long ring_clip_frame(long key, int t, int T, int rate, int rule, long n) {
    const int half = T / 2;
    if (rule == 1) {                                                   // jhmdb: range(start, end), (T - len) / 2 copies of frame 0 in front, `end` behind
        const long start = max(key - half, 0L);
        long end = key + T - half;
        if (n >= 0) end = min(end, n - 1);
        const long len = end - start;                                  // 0 .. T
        const long front = (T - len) / 2;
        if (t < front) return 0;
        if (t < front + len) return start + (t - front);
        return end;
    }
    long f = rule == 0 ? max(key - (long)half * rate, 0L) + (long)t * rate       // ava: the start clamped, then every rate-th frame
                       : key + (long)(t - half) * rate;                          // edge: the key frame stays at position T / 2
    f = max(f, 0L);
    if (n >= 0) f = min(f, n - 1);
    return f;
}

// video_clips_kernel over a ring of the last R frames: frame f sits in slot f % R, frame 0 in the fixed slot R as well (jhmdb pads the clips at
// the END of a video with it).  No index table: key b of the batch is first_key + min(b, n_keys - 1) * key_step.
template <bool V4>
__global__ __launch_bounds__(256) void video_clips_ring_kernel(const uint8_t* __restrict__ ring, int R, int H, int W, long first_key, long key_step,
                                                               int n_keys, int B, int T, int rate, int rule, long n_total, int y1, int x1, int h,
                                                               int w, const float* __restrict__ lut, float* __restrict__ out) {
    __shared__ float s_lut[3 * 256];
    for (int i = threadIdx.x; i < 768; i += blockDim.x) s_lut[i] = lut[i];
    __syncthreads();
    const uint8_t* buf_lo = ring;                                      // the R + 1 slots
    const uint8_t* buf_hi = ring + ((long)R + 1) * H * W * 3;
    const int quads = (w + 3) >> 2;
    const long total = (long)B * T * h * quads;
    const long plane = (long)h * w;
    const long cstride = (long)T * plane;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int xq = (int)(i % quads);
        long r = i / quads;
        const int y = (int)(r % h); r /= h;
        const int t = (int)(r % T), b = (int)(r / T);
        const long f = ring_clip_frame(first_key + (long)min(b, n_keys - 1) * key_step, t, T, rate, rule, n_total);
        const long slot = f <= 0 ? (long)R : f % R;
        const uint8_t* p = ring + (((slot * H + y1 + y) * W) + x1 + xq * 4) * 3;
        float* o = out + ((long)b * 3 * T + t) * plane + (long)y * w + xq * 4;
        video_clips_quad<V4>(p, buf_lo, buf_hi, s_lut, o, cstride, w - xq * 4);
    }
}

}  // namespace

extern "C" {

// The clips of B key frames gathered from a resident video.  frames: uint8 [nframes][H][W][3], packed, at any byte alignment; index: DEVICE
// int32 [B][T], clamped to [0, nframes - 1] by the kernel; (y1, x1, h, w): the window of every frame that is taken; lut: fp32 [3][256]
// (input_pipeline.normalize_lut); out: fp32 [B][3][T][h][w].  A null pointer, a non-positive size or a window outside H x W: TUBER_EINVAL,
// nothing launched.
int tuber_video_clips(const void* frames, int nframes, int H, int W, const int* index, int B, int T, int y1, int x1, int h, int w,
                      const float* lut, float* out, hipStream_t stream) {
    if (!frames || !index || !lut || !out) return TUBER_EINVAL;
    if (nframes <= 0 || H <= 0 || W <= 0 || B <= 0 || T <= 0 || h <= 0 || w <= 0) return TUBER_EINVAL;
    if (y1 < 0 || x1 < 0 || (long)y1 + h > H || (long)x1 + w > W) return TUBER_EINVAL;
    if ((long)B * T > 0x7FFFFFFFl) return TUBER_EINVAL;
    const long total = (long)B * T * h * ((w + 3) / 4);
    const int blocks = (int)min((total + 255) / 256, 65536L * 16);
    if (w % 4 == 0 && ((uintptr_t)out & 15) == 0)
        video_clips_kernel<true><<<blocks, 256, 0, stream>>>((const uint8_t*)frames, nframes, H, W, index, B, T, y1, x1, h, w, lut, out);
    else
        video_clips_kernel<false><<<blocks, 256, 0, stream>>>((const uint8_t*)frames, nframes, H, W, index, B, T, y1, x1, h, w, lut, out);
    TUBER_RETURN_LAUNCH();
}

// tuber_video_clips over a ring of the last R frames (video.VideoStream): ring uint8 [R + 1][H][W][3], packed, at any byte alignment; frame f in
// slot f % R, frame 0 in slot R.  Key b of the batch: first_key + min(b, n_keys - 1) * key_step; rule 0 ava / 1 jhmdb / 2 edge
// (video.clip_indices, evaluated in the kernel); n_total: the video's frame count, < 0 while it is not known.  The caller guarantees that
// every frame a key needs is in the ring.  A null pointer, a non-positive size, R < 1, a negative key, an unknown rule or a window outside H x W:
// TUBER_EINVAL, nothing launched.
int tuber_video_clips_ring(const void* ring, int R, int H, int W, long first_key, long key_step, int n_keys, int B, int T, int rate, int rule,
                           long n_total, int y1, int x1, int h, int w, const float* lut, float* out, hipStream_t stream) {
    if (!ring || !lut || !out) return TUBER_EINVAL;
    if (R < 1 || H <= 0 || W <= 0 || B <= 0 || T <= 0 || rate <= 0 || n_keys <= 0 || h <= 0 || w <= 0) return TUBER_EINVAL;
    if (rule < 0 || rule > 2 || first_key < 0 || key_step < 0 || n_total == 0) return TUBER_EINVAL;
    if (y1 < 0 || x1 < 0 || (long)y1 + h > H || (long)x1 + w > W) return TUBER_EINVAL;
    if ((long)B * T > 0x7FFFFFFFl) return TUBER_EINVAL;
    if (first_key > (1L << 40) || key_step > (1L << 40) || (long)T * rate > 0x7FFFFFFFl) return TUBER_EINVAL;      // frame numbers stay far inside a long
    const long total = (long)B * T * h * ((w + 3) / 4);
    const int blocks = (int)min((total + 255) / 256, 65536L * 16);
    if (w % 4 == 0 && ((uintptr_t)out & 15) == 0)
        video_clips_ring_kernel<true><<<blocks, 256, 0, stream>>>((const uint8_t*)ring, R, H, W, first_key, key_step, n_keys, B, T, rate, rule, n_total,
                                                                  y1, x1, h, w, lut, out);
    else
        video_clips_ring_kernel<false><<<blocks, 256, 0, stream>>>((const uint8_t*)ring, R, H, W, first_key, key_step, n_keys, B, T, rate, rule, n_total,
                                                                   y1, x1, h, w, lut, out);
    TUBER_RETURN_LAUNCH();
}

}  // extern "C"
