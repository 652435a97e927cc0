// Frame-mAP of the validation loop on the device (gfx950): the two kernels behind device_map.py.  They restate evaluation.FrameMAP
// (STDetectionEvaluater, evaluates/evaluate_ava.py:17-171 over the PASCAL evaluator evaluates/utils/object_detection_evaluation.py:309,
// per_image_evaluation.py:354-366,445-449, metrics.py:56-57 + compute_average_precision) with ONE defined rule for equal scores -- they
// keep store order (frame ascending, then row) -- where the reference inherits the permutation of numpy's unstable sort.
//   1. frame_match_kernel   a workgroup per frame, lanes over classes: greedy score-ordered matching of the frame's detections against its
//                           ground-truth boxes, per class; writes one flag per (row, class): 1 true positive, 0 false positive, 2 not counted
//                           (a box with x1 >= x2 or y1 >= y2, a class outside the mask), 3 a frame beyond the kernel's bounds (nothing decided)
//   1b. frame_match_top1_kernel  the JHMDB / UCF101-24 counting rule (evaluation.FrameMAPUCF, evaluates/evaluate_ucf.py:109-126): a row counts once,
//                           as its arg-max class; a wave per frame, a lane per detection, the matching in closed form (no sequential pass)
//   2. ranked_ap_kernel     a workgroup per class over that class's flags in rank order: VOC average precision (area under the monotone
//                           precision envelope) in fp64 from two sweeps over 4096-entry chunks with carries
// No atomics, fixed reduction trees: the same input gives the same bits.  Both are bound by their flag / score traffic, not by arithmetic.
#include "map_common.h"          // FMAP_MAX_DETS / FMAP_MAX_GT, fmap_iou, fmap_key, fmap_argmax: shared with tube_map.hip
#include <float.h>

#define FMAP_THREADS 128          // two waves: C = 80 classes in one trip
#define FMAP_NOT_COUNTED 2
#define FMAP_BEYOND_BOUNDS 3

#define RAP_THREADS 256
#define RAP_PER 16                // flags per thread and chunk: one 16-byte load where the row is aligned
#define RAP_CHUNK (RAP_THREADS * RAP_PER)

__global__ __launch_bounds__(FMAP_THREADS) void frame_match_kernel(const float* __restrict__ det_box, const float* __restrict__ det_score,
                                                                   const int* __restrict__ det_off, const double* __restrict__ gt_box,
                                                                   const unsigned char* __restrict__ gt_lab, const int* __restrict__ gt_off,
                                                                   const unsigned char* __restrict__ class_mask, int N, int G, int C,
                                                                   double iou_thr, unsigned char* __restrict__ flags) {
    __shared__ double iou[FMAP_MAX_DETS * FMAP_MAX_GT];
    __shared__ unsigned long long s_valid;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int d0 = det_off[f], d1 = det_off[f + 1], g0 = gt_off[f], g1 = gt_off[f + 1];
    if (d0 < 0 || d1 < d0 || d1 > N || g0 < 0 || g1 < g0 || g1 > G) return;       // not a CSR row of these arrays: touch nothing
    const int n = d1 - d0, g = g1 - g0;
    if (n > FMAP_MAX_DETS || g > FMAP_MAX_GT) {                                   // the caller's bookkeeping should have kept this frame away
        for (long i = tid; i < (long)n * C; i += FMAP_THREADS) flags[(long)d0 * C + i] = FMAP_BEYOND_BOUNDS;
        return;
    }
    if (n == 0) return;
    if (tid < 64) {                                                               // wave 0: which boxes are boxes (per_image_evaluation.py:445-449)
        bool ok = false;
        if (tid < n) {
            const float* d = det_box + (long)(d0 + tid) * 4;
            ok = d[0] < d[2] && d[1] < d[3];
        }
        const unsigned long long v = __ballot(ok);
        if (tid == 0) s_valid = v;
    }
    for (int p = tid; p < n * g; p += FMAP_THREADS) {
        const int i = p / g, j = p - i * g;
        iou[i * FMAP_MAX_GT + j] = fmap_iou(det_box + (long)(d0 + i) * 4, gt_box + (long)(g0 + j) * 4);
    }
    __syncthreads();
    const unsigned long long valid = s_valid;
    const int nvalid = __popcll(valid);
    for (int c = tid; c < C; c += FMAP_THREADS) {
        const bool wanted = class_mask ? class_mask[c] != 0 : true;
        const float* sc = det_score + (long)d0 * C + c;
        unsigned char* fl = flags + (long)d0 * C + c;
        for (int k = 0; k < n; ++k)
            if (!wanted || !((valid >> k) & 1ull)) fl[(long)k * C] = FMAP_NOT_COUNTED;
        if (!wanted) continue;
        unsigned cand = 0u, taken = 0u;
        for (int j = 0; j < g; ++j)
            if (gt_lab[(long)(g0 + j) * C + c]) cand |= 1u << j;
        unsigned long long last = ~0ull;
        for (int step = 0; step < nvalid; ++step) {
            unsigned long long best = 0ull;                                       // every key is > 0 (its low word is >= ~63)
            for (int k = 0; k < n; ++k) {
                if (!((valid >> k) & 1ull)) continue;
                const unsigned long long key = fmap_key(sc[(long)k * C], k);
                if (key < last && key > best) best = key;
            }
            last = best;
            const int i = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
            unsigned char tp = 0;
            if (cand) {
                int bj = -1;                                                      // np.argmax: the first maximum, a NaN counting as one
                double bv = 0.0;
                for (int j = 0; j < g; ++j) {
                    if (!((cand >> j) & 1u)) continue;
                    const double v = iou[i * FMAP_MAX_GT + j];
                    if (bj < 0 || (bv == bv && (v > bv || v != v))) { bj = j; bv = v; }
                }
                if (bv >= iou_thr && !((taken >> bj) & 1u)) { taken |= 1u << bj; tp = 1; }
            }
            fl[(long)i * C] = tp;
        }
    }
}

#define FTOP_WAVES 4              // frames per workgroup: a wave each

// The UCF counting rule: a row is ONE detection, of its arg-max class a over the C + 1 columns (np.argmax: the first maximum, a NaN counting as
// one), scored det_prob[r][a]; it is not counted when a is the no-object column C, when its box is not a box, or when its frame is on the
// exclude list.  The greedy matching in closed form: the best candidate (bj, bv) of a row -- first arg-max of the IoU over the frame's
// ground-truth rows of class a -- does not depend on the visiting order, and the sequential pass marks a box taken exactly when a row with
// that best candidate and bv >= thr visits it first.  So a row is a true positive iff bv >= thr and no other counted row of the frame with
// the same bj and bv >= thr has a larger order key (keys are distinct: their low word is the row).  A ground-truth row has one class, so an
// equal bj implies an equal class.  Cross-lane reads over the wave; no LDS, no atomics.
__global__ __launch_bounds__(64 * FTOP_WAVES) void frame_match_top1_kernel(const float* __restrict__ det_box, const float* __restrict__ det_prob,
                                                                           const int* __restrict__ det_off, const double* __restrict__ gt_box,
                                                                           const int* __restrict__ gt_cls, const int* __restrict__ gt_off,
                                                                           const unsigned char* __restrict__ frame_skip, int F, int N, int G, int C,
                                                                           double iou_thr, int* __restrict__ det_cls,
                                                                           unsigned char* __restrict__ det_flag) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * FTOP_WAVES + (threadIdx.x >> 6);                   // wave-uniform from here on
    if (f >= F) return;
    const int d0 = det_off[f], d1 = det_off[f + 1], g0 = gt_off[f], g1 = gt_off[f + 1];
    if (d0 < 0 || d1 < d0 || d1 > N || g0 < 0 || g1 < g0 || g1 > G) return;       // not a CSR row of these arrays: touch nothing
    const int n = d1 - d0, g = g1 - g0;
    if (n > FMAP_MAX_DETS || g > FMAP_MAX_GT) {
        for (int i = lane; i < n; i += 64) {
            det_cls[d0 + i] = -1;
            det_flag[d0 + i] = FMAP_BEYOND_BOUNDS;
        }
        return;
    }
    if (n == 0) return;
    const bool skip = frame_skip ? frame_skip[f] != 0 : false;
    const bool have = lane < n;
    int a = C;
    float score = 0.f;
    bool counted = false;
    int bj = -1;
    bool hit = false;
    if (have) {
        const float* p = det_prob + (long)(d0 + lane) * (C + 1);
        a = fmap_argmax(p, C, score);
        const float* d = det_box + (long)(d0 + lane) * 4;
        counted = a != C && d[0] < d[2] && d[1] < d[3] && !skip;
        if (counted) {
            double bv = 0.0;
            for (int j = 0; j < g; ++j) {                                         // the ground truth is read uniformly: the same address in every lane
                if (gt_cls[g0 + j] != a) continue;
                const double v = fmap_iou(d, gt_box + (long)(g0 + j) * 4);
                if (bj < 0 || (bv == bv && (v > bv || v != v))) { bj = j; bv = v; }
            }
            hit = bj >= 0 && bv >= iou_thr;
        }
    }
    const unsigned long long key = fmap_key(score, lane);
    const int claim = hit ? bj : -1;                                              // the box this row would take
    bool lost = false;
    for (int m = 0; m < n; ++m) {                                                 // every lane of the wave is here: m is uniform
        const int cm = __shfl(claim, m, 64);
        const unsigned long long km = __shfl(key, m, 64);
        lost |= cm == claim && km > key;
    }
    if (have) {
        det_cls[d0 + lane] = a;
        det_flag[d0 + lane] = !counted ? (unsigned char)FMAP_NOT_COUNTED : (unsigned char)((hit && !lost) ? 1 : 0);
    }
}

__device__ __forceinline__ void rap_load(const unsigned char* __restrict__ row, long base, long N, bool vec, unsigned char (&v)[RAP_PER]) {
    if (vec && base + RAP_PER <= N) {
        const uint4 q = *(const uint4*)(row + base);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < RAP_PER; ++e) v[e] = (unsigned char)((w[e >> 2] >> ((e & 3) * 8)) & 0xFFu);
    } else {
#pragma unroll
        for (int e = 0; e < RAP_PER; ++e) v[e] = base + e < N ? row[base + e] : (unsigned char)FMAP_NOT_COUNTED;
    }
}

// One class: flags in rank order -> AP.  With ctp_i / cfp_i the counted true / false positives up to rank i, precision_i = ctp_i /
// max(ctp_i + cfp_i, DBL_EPSILON), recall_i = ctp_i / n_gt: AP = sum over the true positives of (recall_i - recall_before) * max_{j >= i}
// precision_j -- evaluation._average_precision, whose recall changes exactly at the true positives and whose envelope ends in 0.
// Sweep 1 counts (integers: any order).  Sweep 2 walks the chunks from the last to the first: the counts up to a chunk's start are the
// remaining totals minus the chunk's own, the envelope arrives as a carry from the chunks behind, and the chunk's terms are added in a fixed
// tree, the chunks in descending order.
__global__ __launch_bounds__(RAP_THREADS) void ranked_ap_kernel(const unsigned char* __restrict__ flags, const int* __restrict__ n_gt, long N,
                                                                double* __restrict__ ap, int* __restrict__ n_tp) {
    __shared__ unsigned long long s_cnt[RAP_THREADS / 64];
    __shared__ double s_max[RAP_THREADS / 64];
    __shared__ double s_sum[RAP_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned char* row = flags + (long)c * N;
    const bool vec = (((uintptr_t)row) & 15) == 0;
    const int ng = n_gt[c];
    unsigned char v[RAP_PER];

    // sweep 1: totals, true positives in the high word
    unsigned long long cnt = 0ull;
    for (long base = (long)tid * RAP_PER; base < N; base += RAP_CHUNK) {
        rap_load(row, base, N, vec, v);
#pragma unroll
        for (int e = 0; e < RAP_PER; ++e) cnt += v[e] == 1 ? (1ull << 32) : (v[e] == 0 ? 1ull : 0ull);
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) cnt += __shfl_xor(cnt, s, 64);
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    const unsigned long long total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
    if (tid == 0 && n_tp) n_tp[c] = (int)(total >> 32);
    if (ng <= 0) {
        if (tid == 0) ap[c] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    if (total == 0ull) {
        if (tid == 0) ap[c] = 0.0;
        return;
    }

    const double dng = (double)ng;
    unsigned long long rem = total;                    // counted entries in [0, end of the current chunk)
    double carry = 0.0, acc = 0.0;                     // envelope behind the current chunk; the sum so far (the same in every thread)
    const long nchunks = (N + RAP_CHUNK - 1) / RAP_CHUNK;
    for (long ch = nchunks - 1; ch >= 0; --ch) {
        rap_load(row, ch * RAP_CHUNK + (long)tid * RAP_PER, N, vec, v);
        unsigned long long mine = 0ull;
#pragma unroll
        for (int e = 0; e < RAP_PER; ++e) mine += v[e] == 1 ? (1ull << 32) : (v[e] == 0 ? 1ull : 0ull);
        unsigned long long incl = mine;                // inclusive scan over the threads of the chunk
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned long long t = __shfl_up(incl, s, 64);
            if (lane >= s) incl += t;
        }
        if (lane == 63) s_cnt[wv] = incl;
        __syncthreads();
        unsigned long long before = 0ull, chunk_total = 0ull;
#pragma unroll
        for (int w = 0; w < RAP_THREADS / 64; ++w) {
            if (w < wv) before += s_cnt[w];
            chunk_total += s_cnt[w];
        }
        unsigned long long pre = rem - chunk_total + before + incl - mine;      // counted entries in front of this thread's first flag
        double prec[RAP_PER], dr[RAP_PER];
        double tmax = 0.0;
#pragma unroll
        for (int e = 0; e < RAP_PER; ++e) {
            prec[e] = -1.0;
            dr[e] = 0.0;
            if (v[e] == 1) {
                pre += 1ull << 32;
                const double ctp = (double)(unsigned)(pre >> 32), cfp = (double)(unsigned)(pre & 0xFFFFFFFFull);
                prec[e] = ctp / fmax(ctp + cfp, DBL_EPSILON);
                dr[e] = ctp / dng - (ctp - 1.0) / dng;
                tmax = fmax(tmax, prec[e]);
            } else if (v[e] == 0) {
                pre += 1ull;
            }
        }
        double suf = tmax;                             // inclusive suffix maximum over the threads of the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const double t = __shfl_down(suf, s, 64);
            if (lane + s < 64) suf = fmax(suf, t);
        }
        if (lane == 0) s_max[wv] = suf;
        double env = __shfl_down(suf, 1, 64);          // the threads behind this one in the wave
        if (lane == 63) env = 0.0;
        __syncthreads();
        double chunk_max = 0.0;
#pragma unroll
        for (int w = 0; w < RAP_THREADS / 64; ++w) {
            if (w > wv) env = fmax(env, s_max[w]);
            chunk_max = fmax(chunk_max, s_max[w]);
        }
        env = fmax(env, carry);
        double sum = 0.0;
#pragma unroll
        for (int e = RAP_PER - 1; e >= 0; --e) {
            if (prec[e] >= 0.0) {
                env = fmax(env, prec[e]);
                sum += dr[e] * env;
            }
        }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) sum += __shfl_xor(sum, s, 64);
        if (lane == 0) s_sum[wv] = sum;
        __syncthreads();
        acc += ((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
        carry = fmax(carry, chunk_max);
        rem -= chunk_total;
    }
    if (tid == 0) ap[c] = acc;
}

extern "C" {

// Greedy matching of every (frame, class): rows [det_off[f], det_off[f + 1]) of det_box ([N][4] fp32 xyxy) / det_score ([N][C] fp32) are frame
// f's detections, rows [gt_off[f], gt_off[f + 1]) of gt_box ([G][4] fp64) / gt_lab ([G][C] bytes, non-zero = the box carries that class) its
// ground truth; det_off / gt_off: DEVICE int[F + 1].  class_mask: [C] bytes, zero = class not evaluated (NULL: all).  flags: [N][C] bytes out.
// At most tuber_frame_match_max_dets() detections and tuber_frame_match_max_gt() ground-truth boxes per frame: sizes that cannot meet that
// (N > F * max_dets, G > F * max_gt) are refused here; the caller keeps a single frame beyond a bound away (device_map.py evaluates on the
// host then) -- the kernel marks such a frame's rows 3 and decides nothing for it.
int tuber_frame_match(const float* det_box, const float* det_score, const int* det_off, const double* gt_box, const unsigned char* gt_lab,
                      const int* gt_off, const unsigned char* class_mask, int F, int N, int G, int C, double iou_thr, unsigned char* flags,
                      hipStream_t stream) {
    if (F < 0 || N < 0 || G < 0 || C <= 0 || !(iou_thr == iou_thr)) return TUBER_EINVAL;
    if ((long)N > (long)F * FMAP_MAX_DETS || (long)G > (long)F * FMAP_MAX_GT) return TUBER_EINVAL;
    if (N == 0) return TUBER_OK;
    if (!det_box || !det_score || !det_off || !gt_off || !flags) return TUBER_EINVAL;
    if (G > 0 && (!gt_box || !gt_lab)) return TUBER_EINVAL;
    hipLaunchKernelGGL(frame_match_kernel, dim3(F), dim3(FMAP_THREADS), 0, stream, det_box, det_score, det_off, gt_box, gt_lab, gt_off,
                       class_mask, N, G, C, iou_thr, flags);
    TUBER_RETURN_LAUNCH();
}
int tuber_frame_match_max_dets() { return FMAP_MAX_DETS; }
int tuber_frame_match_max_gt() { return FMAP_MAX_GT; }

// The matching step under the JHMDB / UCF101-24 counting rule (evaluation.FrameMAPUCF): det_prob [N][C + 1] fp32, columns [0, C) the classes and
// column C no-object; gt_cls [G] the 0-based class of a ground-truth row (a class outside [0, C) matches nothing); frame_skip [F] bytes, non-zero =
// the frame is on the exclude list (NULL: none).  det_cls [N] out: the row's arg-max column (C = no-object); det_flag [N] out: 1 true positive,
// 0 false positive, 2 not counted, 3 (with det_cls -1) a frame beyond the bounds.  Offsets, bounds and refusals as tuber_frame_match.
int tuber_frame_match_top1(const float* det_box, const float* det_prob, const int* det_off, const double* gt_box, const int* gt_cls,
                           const int* gt_off, const unsigned char* frame_skip, int F, int N, int G, int C, double iou_thr, int* det_cls,
                           unsigned char* det_flag, hipStream_t stream) {
    if (F < 0 || N < 0 || G < 0 || C <= 0 || !(iou_thr == iou_thr)) return TUBER_EINVAL;
    if ((long)N > (long)F * FMAP_MAX_DETS || (long)G > (long)F * FMAP_MAX_GT) return TUBER_EINVAL;
    if (N == 0) return TUBER_OK;
    if (!det_box || !det_prob || !det_off || !gt_off || !det_cls || !det_flag) return TUBER_EINVAL;
    if (G > 0 && (!gt_box || !gt_cls)) return TUBER_EINVAL;
    hipLaunchKernelGGL(frame_match_top1_kernel, dim3((F + FTOP_WAVES - 1) / FTOP_WAVES), dim3(64 * FTOP_WAVES), 0, stream, det_box, det_prob,
                       det_off, gt_box, gt_cls, gt_off, frame_skip, F, N, G, C, iou_thr, det_cls, det_flag);
    TUBER_RETURN_LAUNCH();
}

// VOC average precision per class from flags in rank order: flags_ranked [C][N] bytes (1 true positive, 0 false positive, anything else counts
// nowhere), n_gt [C] ground-truth boxes of the class -> ap [C] fp64 (NaN where n_gt <= 0, 0.0 where nothing is counted) and n_tp [C] (NULL: not
// wanted).  N == 0 is legal.
int tuber_ranked_ap(const unsigned char* flags_ranked, const int* n_gt, int C, int N, double* ap, int* n_tp, hipStream_t stream) {
    if (C <= 0 || N < 0 || !n_gt || !ap) return TUBER_EINVAL;
    if (N > 0 && !flags_ranked) return TUBER_EINVAL;
    hipLaunchKernelGGL(ranked_ap_kernel, dim3(C), dim3(RAP_THREADS), 0, stream, flags_ranked, n_gt, (long)N, ap, n_tp);
    TUBER_RETURN_LAUNCH();
}

}  // extern "C"
