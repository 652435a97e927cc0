// Crops of action tubes and actor tracks out of the resident video on gfx950 (crops.crop_rows: the definition).
// Row r of a crop table names a frame and a box in source-video pixels; its crop is the box, enlarged by `scale` about its centre, resampled
// to h x w: every output pixel the mean of an s x s regular grid of bilinear samples (RoIAlign's sampling_ratio), the sample positions clamped
// to the frame (edge replication: grid_sample's padding_mode="border", align_corners=False).  All arithmetic is fp64, every operation rounded
// on its own and in the definition's order, so the bytes are the definition's.
//
// A workgroup owns one crop row and a band of LB output lines -- at most TCROP_BAND_BYTES output bytes, so that a lane owns at most two
// aligned dwords of the flat output and keeps their eight fp64 sums in registers.  The coordinates and weights of the w * s sample columns
// and of the band's LB * s sample lines are computed once into LDS tables and shared by the three channels and by the whole band.  Per pass
// dy over the sample lines of an output line, the two source lines of each of the band's sample lines are staged into LDS: only the span
// of columns the box touches (at most 3 * W bytes a line, hence TCROP_MAX_W), read as aligned dwords whatever the byte alignment of a
// frame line (W * 3 is rarely a multiple of 4); the first and the last dword of the frame buffer are taken byte by byte.  Every lane then
// forms its bytes from LDS.  Stores: aligned dwords over the flat uint8 output with a byte head and tail per band (h * w * 3 need not be a
// multiple of 4, so neither a row nor a band starts aligned; neighbouring bands write disjoint bytes of a shared dword); in the table form
// (lut != NULL) fp32 [R][3][h][w], 16 bytes a lane where four pixels of a line are aligned, scalars elsewhere.  No atomics, plain vector
// stores, nothing is written outside the row's h * w * 3 elements and valid[r].
#include "common.h"
#include <math.h>

#define TCROP_THREADS 256
#define TCROP_MAX_W 4096          // frame width: two staged lines of 3 * W bytes and the column table fit the 64 KB of a workgroup
#define TCROP_MAX_OUT 512         // h and w of a crop
#define TCROP_MAX_SAMPLES 4
#define TCROP_BAND_BYTES 2040     // output bytes of a band: at most 511 aligned dwords with head and tail, two per lane
#define TCROP_MAX_LINES 32        // output lines of a band
#define TCROP_LDS 61440           // dynamic LDS a launch may ask for

namespace {

struct CropAxis {
    double origin, step;          // the definition's X1 and sx (Y1 and sy)
};

__device__ __forceinline__ CropAxis crop_axis(float lo, float hi, double f, double scale, int n) {
#pragma clang fp contract(off)
    const double c = ((double)lo + (double)hi) * 0.5;
    const double b = ((double)hi - (double)lo) * scale;
    CropAxis ax;
    ax.origin = (c - b * 0.5) * f;
    ax.step = (b * f) / (double)n;
    return ax;
}

// sample k of an axis over `size` source pixels: the two pixels and the weight of the second.  A NaN position (an overflowing scale) is 0.
__device__ __forceinline__ void crop_coord(CropAxis ax, int k, int size, int& i0, int& i1, double& wgt) {
#pragma clang fp contract(off)
    double u = ax.origin + ((double)k + 0.5) * ax.step - 0.5;
    const double top = (double)(size - 1);
    u = u > 0.0 ? u : 0.0;
    u = u < top ? u : top;
    const double f = floor(u);
    i0 = (int)f;
    i1 = min(i0 + 1, size - 1);
    wgt = u - f;
}

__host__ __device__ __forceinline__ int tcrop_align16(int v) { return (v + 15) & ~15; }
// bytes of the tables in front of the staged lines: per sample column a weight and two byte offsets, per sample line of the band a weight
// and two line numbers, per staged line its byte shift
__host__ __device__ __forceinline__ int tcrop_table_bytes(int ws, int LB, int s) { return ws * 16 + LB * s * 16 + tcrop_align16(2 * LB * 4); }

// where byte q of a band lies: byte form (line, pixel, channel) in memory order, table form (line, channel, pixel)
template <bool LUT>
__device__ __forceinline__ void tcrop_locate(int q, int w, int& il, int& j, int& ch) {
    const int w3 = w * 3;
    il = q / w3;
    const int rem = q - il * w3;
    if (LUT) {
        ch = rem / w;
        j = rem - ch * w;
    } else {
        j = rem / 3;
        ch = rem - j * 3;
    }
}
template <bool LUT>
__device__ __forceinline__ void tcrop_next(int w, int& il, int& j, int& ch) {
    if (LUT) {
        if (++j == w) {
            j = 0;
            if (++ch == 3) { ch = 0; ++il; }
        }
    } else {
        if (++ch == 3) {
            ch = 0;
            if (++j == w) { j = 0; ++il; }
        }
    }
}

template <bool LUT>
__global__ __launch_bounds__(TCROP_THREADS) void tube_crops_kernel(const uint8_t* __restrict__ frames, int N, int H, int W,
                                                                   const int* __restrict__ frame_index, const float* __restrict__ boxes, int h,
                                                                   int w, double fx, double fy, double scale, int s, int LB, int nbands,
                                                                   int linebytes, const float* __restrict__ lut, void* __restrict__ out,
                                                                   uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char tcrop_lds[];
    const int tid = threadIdx.x;
    const long r = blockIdx.x / nbands;                                            // workgroup-uniform from here to the item set-up
    const int band = blockIdx.x - (int)r * nbands;
    const int i_lo = band * LB;
    const int nl = min(LB, h - i_lo);
    const int ws = w * s, w3 = w * 3;
    double* col_a = (double*)tcrop_lds;                                            // [ws] the weight of a sample column's second pixel
    int2* col_o = (int2*)(col_a + ws);                                             // [ws] the byte offsets of its two pixels in a staged line
    double* lin_b = (double*)(col_o + ws);                                         // [LB * s] the weight of a sample line's second source line
    int2* lin_i = (int2*)(lin_b + LB * s);                                         // [LB * s] its two source lines
    int* st_sh = (int*)(lin_i + LB * s);                                           // [2 * LB] the byte shift of a staged line
    uint8_t* stage = tcrop_lds + tcrop_table_bytes(ws, LB, s);                     // [2 * LB][linebytes]

    const int n = frame_index[r];
    const float4 bx = ((const float4*)boxes)[r];
    const bool ok = n >= 0 && n < N && isfinite(bx.x) && isfinite(bx.y) && isfinite(bx.z) && isfinite(bx.w);
    if (band == 0 && tid == 0) valid[r] = ok ? 1 : 0;

    // the band's bytes as items of four: aligned dwords of the flat output (byte form), runs of four from the band's first byte (table form)
    const int nbytes = nl * w3;
    uint8_t* band_out = (uint8_t*)out + (r * h + i_lo) * (long)w3;                 // byte form only
    const int head = LUT ? 0 : (int)((uintptr_t)band_out & 3);
    const int nitems = (head + nbytes + 3) >> 2;
    int it_il[2], it_j[2], it_ch[2];
    double acc[2][4];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int q = max((tid + it * TCROP_THREADS) * 4 - head, 0);
        tcrop_locate<LUT>(q, w, it_il[it], it_j[it], it_ch[it]);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[it][k] = 0.0;
    }

    if (ok) {
        const CropAxis ax = crop_axis(bx.x, bx.z, fx, scale, ws), ay = crop_axis(bx.y, bx.w, fy, scale, h * s);
        int ja0, ja1, jb0, jb1;
        double unused;
        crop_coord(ax, 0, W, ja0, ja1, unused);                                    // the positions are monotone in the column: the ends bound the span
        crop_coord(ax, ws - 1, W, jb0, jb1, unused);
        const int jmin = min(ja0, jb0), jmax = max(ja1, jb1);
        const int span = (jmax - jmin + 1) * 3;
        const int ndmax = (span + 6) >> 2;                                         // dwords of a staged line at the largest shift
        for (int c = tid; c < ws; c += TCROP_THREADS) {
            int j0, j1;
            double a;
            crop_coord(ax, c, W, j0, j1, a);
            col_a[c] = a;
            col_o[c] = make_int2((j0 - jmin) * 3, (j1 - jmin) * 3);
        }
        for (int k = tid; k < nl * s; k += TCROP_THREADS) {
            int i0, i1;
            double b;
            crop_coord(ay, i_lo * s + k, H, i0, i1, b);
            lin_b[k] = b;
            lin_i[k] = make_int2(i0, i1);
        }
        const uint8_t* buf_lo = frames;                                            // [buf_lo, buf_hi): the bytes of `frames` that may be touched
        const uint8_t* buf_hi = frames + (long)N * H * W * 3;
        for (int dy = 0; dy < s; ++dy) {
            __syncthreads();                                                       // the tables are written; the last pass has read its lines
            for (int idx = tid; idx < 2 * nl * ndmax; idx += TCROP_THREADS) {
                const int line = idx / ndmax, d = idx - line * ndmax;
                const int2 ii = lin_i[(line >> 1) * s + dy];
                const uint8_t* g0 = frames + (((long)n * H + ((line & 1) ? ii.y : ii.x)) * W + jmin) * 3;
                const int sh = (int)((uintptr_t)g0 & 3);
                if (d == 0) st_sh[line] = sh;
                if (d * 4 < sh + span) {
                    const uint8_t* g = g0 - sh + 4 * d;
                    uint32_t v = 0;
                    if (g >= buf_lo && g + 4 <= buf_hi) v = *(const uint32_t*)g;
                    else {
                        for (int e = 0; e < 4; ++e)
                            if (g + e >= buf_lo && g + e < buf_hi) v |= (uint32_t)g[e] << (8 * e);
                    }
                    *(uint32_t*)(stage + line * linebytes + 4 * d) = v;
                }
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int t = tid + it * TCROP_THREADS;
                if (t < nitems) {
                    const int qs = t * 4 - head;
                    int il = it_il[it], j = it_j[it], ch = it_ch[it];
                    // an item's four bytes mostly share a line, and with s = 1 a pixel's three a column: the table entries are read when they change
                    int line = -1, column = -1;
                    double b = 0.0, a = 0.0;
                    int2 o = make_int2(0, 0);
                    const uint8_t *top0 = stage, *bot0 = stage;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (qs + k >= 0 && qs + k < nbytes) {
                            if (il != line) {
                                line = il;
                                b = lin_b[il * s + dy];
                                top0 = stage + (2 * il) * linebytes + st_sh[2 * il];
                                bot0 = stage + (2 * il + 1) * linebytes + st_sh[2 * il + 1];
                            }
                            const uint8_t *top = top0 + ch, *bot = bot0 + ch;
                            double sum = acc[it][k];
                            for (int dx = 0; dx < s; ++dx) {
                                const int c = j * s + dx;
                                if (c != column) {
                                    column = c;
                                    a = col_a[c];
                                    o = col_o[c];
                                }
                                // the difference of two bytes is exact as an integer and as a double: one conversion, no fp64 subtraction
                                const int q00 = top[o.x], q10 = bot[o.x];
                                const double p00 = (double)q00, p10 = (double)q10;
                                const double tp = p00 + (double)((int)top[o.y] - q00) * a;
                                const double bt = p10 + (double)((int)bot[o.y] - q10) * a;
                                sum = sum + (tp + (bt - tp) * b);
                            }
                            acc[it][k] = sum;
                            tcrop_next<LUT>(w, il, j, ch);
                        }
                    }
                }
            }
        }
    }

    // acc / (s * s): for s = 1, 2, 4 the product with the exact reciprocal, which rounds the same quotient; a division for s = 3
    const double count = (double)(s * s);
    const bool pow2 = (s & (s - 1)) == 0;
    const double inv = 1.0 / count;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int t = tid + it * TCROP_THREADS;
        if (t >= nitems) continue;
        const int qs = t * 4 - head;
        uint32_t bytes[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) bytes[k] = (uint32_t)floor((pow2 ? acc[it][k] * inv : acc[it][k] / count) + 0.5);
        const bool whole = qs >= 0 && qs + 4 <= nbytes;
        if (!LUT) {
            uint8_t* o = band_out + qs;
            if (whole) *(uint32_t*)o = bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (qs + k >= 0 && qs + k < nbytes) o[k] = (uint8_t)bytes[k];
            }
        } else {
            int il = it_il[it], j = it_j[it], ch = it_ch[it];
            float* o = (float*)out + ((r * 3 + ch) * h + i_lo + il) * (long)w + j;
            if (whole && j + 4 <= w && ((uintptr_t)o & 15) == 0) {
                const float* l = lut + ch * 256;
                *(float4*)o = make_float4(l[bytes[0]], l[bytes[1]], l[bytes[2]], l[bytes[3]]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (qs + k < nbytes) {
                        ((float*)out)[((r * 3 + ch) * h + i_lo + il) * (long)w + j] = lut[ch * 256 + bytes[k]];
                        tcrop_next<LUT>(w, il, j, ch);
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" {

// Crops of tubes and tracks out of a resident video (crops.crop_rows: the definition).  frames: uint8 [N][H][W][3], packed, at any byte
// alignment; frame_index int32 [R] and boxes fp32 [R][4] (xyxy in source pixels, pixel j covering [j, j + 1)): the crop table; fx = W / W0,
// fy = H / H0: the host's fp64 quotients of the frame size by the size the boxes refer to; scale > 0 enlarges a box about its centre;
// samples = s: an output pixel is the mean of s x s bilinear samples.  Per axis, in fp64, every operation rounded on its own:
//     cx = (x1 + x2) * 0.5; bw = (x2 - x1) * scale; X1 = (cx - bw * 0.5) * fx; sx = (bw * fx) / double(w * s)
//     sample column c: u = X1 + (c + 0.5) * sx - 0.5, clamped to [0, W - 1] (a NaN to 0); j0 = floor(u); j1 = min(j0 + 1, W - 1); a = u - j0
//     top = p[i0][j0] + (p[i0][j1] - p[i0][j0]) * a; bot likewise on line i1; val = top + (bot - top) * b
//     pixel (i, j): acc = 0; for dy, for dx: acc = acc + val(i * s + dy, j * s + dx); byte = floor(acc / double(s * s) + 0.5)
// lut == NULL: out is uint8 [R][h][w][3], at any byte alignment.  lut != NULL: fp32 [3][256], the table of tuber_video_clips
// (input_pipeline.normalize_lut), and out is fp32 [R][3][h][w] with out[r][ch][i][j] = lut[ch][byte].  valid uint8 [R]: 0 at a row whose
// frame_index lies outside [0, N) or whose box has a coordinate that is not finite; such a row's bytes are 0.  x2 < x1 mirrors, a box of no
// area gives a constant: the formula decides.  Refused (TUBER_EINVAL, nothing launched, nothing written): W > tuber_tube_crops_limits(0), h
// or w > limits(1), samples > limits(2); h, w, samples, H or W below 1; negative N or R; R * bands of lines beyond an int32; fx, fy or scale
// not finite or not positive; a null pointer; boxes not 16-byte, frame_index not 4-byte, lut or an fp32 out not 4-byte aligned.  R == 0:
// TUBER_OK, no launch, the pointers are not inspected.
int tuber_tube_crops(const unsigned char* frames, int N, int H, int W, const int* frame_index, const float* boxes, int R, int h, int w, double fx,
                     double fy, double scale, int samples, const float* lut, void* out, unsigned char* valid, hipStream_t stream) {
    if (N < 0 || R < 0 || H < 1 || W < 1 || h < 1 || w < 1 || samples < 1) return TUBER_EINVAL;
    if (W > TCROP_MAX_W || h > TCROP_MAX_OUT || w > TCROP_MAX_OUT || samples > TCROP_MAX_SAMPLES) return TUBER_EINVAL;
    if (!(fx > 0.0) || !(fy > 0.0) || !(scale > 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(scale)) return TUBER_EINVAL;
    if (R == 0) return TUBER_OK;
    if (!frames || !frame_index || !boxes || !out || !valid) return TUBER_EINVAL;
    if (((uintptr_t)boxes & 15) || ((uintptr_t)frame_index & 3) || ((uintptr_t)lut & 3) || (lut && ((uintptr_t)out & 3))) return TUBER_EINVAL;
    // the band: as many output lines as TCROP_BAND_BYTES and the LDS hold
    const int linebytes = tcrop_align16(3 * W + 8);
    int LB = TCROP_BAND_BYTES / (w * 3);
    LB = LB < 1 ? 1 : LB;
    LB = LB > h ? h : LB;
    LB = LB > TCROP_MAX_LINES ? TCROP_MAX_LINES : LB;
    while (LB > 1 && (long)tcrop_table_bytes(w * samples, LB, samples) + 2l * LB * linebytes > TCROP_LDS) --LB;
    const size_t lds = (size_t)tcrop_table_bytes(w * samples, LB, samples) + 2 * (size_t)LB * linebytes;
    const int nbands = (h + LB - 1) / LB;
    if ((long)R * nbands > 0x7FFFFFFFl) return TUBER_EINVAL;
    const dim3 grid((unsigned)((long)R * nbands));
    if (lut)
        hipLaunchKernelGGL(tube_crops_kernel<true>, grid, dim3(TCROP_THREADS), lds, stream, frames, N, H, W, frame_index, boxes, h, w, fx, fy, scale, samples,
                           LB, nbands, linebytes, lut, out, valid);
    else
        hipLaunchKernelGGL(tube_crops_kernel<false>, grid, dim3(TCROP_THREADS), lds, stream, frames, N, H, W, frame_index, boxes, h, w, fx, fy, scale, samples,
                           LB, nbands, linebytes, lut, out, valid);
    TUBER_RETURN_LAUNCH();
}

// bounds of tuber_tube_crops: which = 0 the largest W, 1 the largest h or w, 2 the largest samples; anything else -1
int tuber_tube_crops_limits(int which) { return which == 0 ? TCROP_MAX_W : which == 1 ? TCROP_MAX_OUT : which == 2 ? TCROP_MAX_SAMPLES : -1; }

}  // extern "C"
