// Ranked detections from the raw head outputs of an eval forward (gfx950): ONE launch per batch, one workgroup per clip.  The two kernels restate
// the post-processors (PostProcessAVA, models/criterion.py:447-482; PostProcess, models/tuber_jhmdb.py:357-389; criterion.py's decode() methods
// here) followed by what a caller who wants boxes, labels and scores does by hand: threshold, (arg-max,) top-K, in one defined order.
//   detect_kernel<0>   AVA rule: pb = softmax(logits_b)[1]; a query passes the gate when pb > actor_thr; score(q, c) = sigmoid(logit) * pb; a candidate
//                      is a (q, c) of a gated query whose score is not NaN and >= score_thr; order: score descending, then q, then c ascending
//   detect_kernel<1>   JHMDB / UCF101-24 rule (counted once, evaluates/evaluate_ucf.py:109-126): a query's label is the first maximum of its fp32 logit
//                      row over the C + 1 columns (a NaN counting as a maximum, fmap_argmax), its score that column's softmax probability; not a
//                      candidate when the label is the no-object column C, the score is NaN or < score_thr; order: score descending, then q ascending
//   detect_actors_kernel   AVA rule per ACTOR (tuber_detect_actors): the queries with pb > actor_thr ranked by pb descending, then q ascending, the best A kept,
//                      each with its box and its whole action row sigmoid(logit) * pb -- detect_kernel<0>'s score of every (q, c), unthresholded
// The candidates' order keys (fmap_key: the score as an order-preserving unsigned over ~index) sit in LDS, non-candidates as key 0, and a bitonic
// network sorts them descending: keys are distinct, so the result is a function of the inputs alone -- no atomics anywhere.  The score is recovered
// from the key's high word bit for bit.  Inputs are read in the dtype the forward produced (fp32 or bf16, converted on load: no cast launch).
// Boxes are box_ops.box_cxcywh_to_xyxy and the multiply by (W, H, W, H), expression for expression in fp32 without contraction (this source is built
// with -ffp-contract=on, under which the pragma holds): bit-identical to decode()'s.
#include "map_common.h"

#define DET_THREADS 512
#define DET_MAX_KEYS 4096         // Qs * C: the clip's keys are 32 KB of LDS
#define DET_MAX_K 1024
#define DET_MAX_NB 8              // columns of logits_b (3 for AVA, 2 for JHMDB / UCF101-24)
#define DET_EBOUNDS (-2)          // a legal call beyond the kernel's bounds: nothing launched, the caller decodes another way

#define DET_BF16_LOGITS 1
#define DET_BF16_LOGITS_B 2
#define DET_BF16_BOXES 4

__device__ __forceinline__ float det_ld(const void* __restrict__ p, long i, bool bf) {
    return bf ? bf2f(((const bf16*)p)[i]) : ((const float*)p)[i];
}

// softmax(row)[1] over nb columns, fp32: exp(x - max) / sum in column order, as a row-wise softmax evaluates it
__device__ __forceinline__ float det_prob1(const void* __restrict__ lb, long row, int nb, bool bf) {
    float x[DET_MAX_NB];
    float m = -INFINITY;
    bool nan = false;
    for (int j = 0; j < nb; ++j) {
        x[j] = det_ld(lb, row * nb + j, bf);
        nan |= x[j] != x[j];
        m = fmaxf(m, x[j]);
    }
    if (nan) return NAN;
    float sum = 0.f, e1 = 0.f;
    for (int j = 0; j < nb; ++j) {
        const float e = expf(x[j] - m);
        sum += e;
        if (j == 1) e1 = e;
    }
    return e1 / sum;
}

// the score back from an order key's high word (fmap_key's map inverted; -0 went in as +0, NaN never gets here)
__device__ __forceinline__ float det_score_of(unsigned long long key) {
    const unsigned u = (unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

template <int TOP1>
__global__ __launch_bounds__(DET_THREADS) void detect_kernel(const void* __restrict__ logits, const void* __restrict__ logits_b,
                                                             const void* __restrict__ boxes, const float* __restrict__ sizes,
                                                             const int* __restrict__ q_begin, int Qtot, int Qs, int C, int NB, int lb_rows,
                                                             int dtypes, float actor_thr, float score_thr, int K, float* __restrict__ det_box,
                                                             float* __restrict__ det_score, int* __restrict__ det_label,
                                                             int* __restrict__ det_query, float* __restrict__ det_aux,
                                                             int* __restrict__ det_count, int* __restrict__ det_total) {
    __shared__ unsigned long long keys[DET_MAX_KEYS];
    __shared__ float s_pb[TOP1 ? 1 : DET_MAX_KEYS];     // AVA: a query's actor probability; top1: the clip's visibility probability
    __shared__ int s_lab[TOP1 ? DET_MAX_KEYS : 1];      // top1: a query's arg-max column (48 KB of LDS either way)
    __shared__ int s_cnt[DET_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool bf_lg = dtypes & DET_BF16_LOGITS, bf_lb = dtypes & DET_BF16_LOGITS_B, bf_bx = dtypes & DET_BF16_BOXES;
    const int CW = TOP1 ? C + 1 : C;                    // columns of a logit row
    const int N = TOP1 ? Qs : Qs * C;                   // keys of the clip
    int n2 = 2;
    while (n2 < N) n2 <<= 1;                            // <= DET_MAX_KEYS (the launcher checked N)
    int q0 = q_begin ? q_begin[b] : 0;
    const bool slice_ok = q0 >= 0 && q0 <= Qtot - Qs;   // a slice outside the clip's queries: an empty result, nothing read
    if (!slice_ok) q0 = 0;
    const long qrow0 = (long)b * Qtot + q0;             // first row of the slice in [B * Qtot]

    // ---- per query: actor / visibility probability (and, top1, label and score) ----
    if (TOP1) {
        if (tid == 0) s_pb[0] = lb_rows == 1 ? det_prob1(logits_b, b, NB, bf_lb) : 0.f;
    }
    int mine = 0;                                       // candidates this thread found
    if (!TOP1) {
        for (int q = tid; q < Qs; q += DET_THREADS)
            s_pb[q] = slice_ok ? det_prob1(logits_b, lb_rows == 1 ? (long)b : qrow0 + q, NB, bf_lb) : 0.f;
        __syncthreads();
        for (int i = tid; i < n2; i += DET_THREADS) {
            unsigned long long key = 0ull;
            if (i < N && slice_ok) {
                const int q = i / C, c = i - q * C;
                const float pb = s_pb[q];
                if (pb > actor_thr) {
                    const float x = det_ld(logits, (qrow0 + q) * C + c, bf_lg);
                    const float s = (1.f / (1.f + expf(-x))) * pb;
                    if (s == s && s >= score_thr) { key = fmap_key(s, i); ++mine; }
                }
            }
            keys[i] = key;
        }
    } else {
        for (int q = tid; q < n2; q += DET_THREADS) {
            unsigned long long key = 0ull;
            if (q < N && slice_ok) {
                const long base = (qrow0 + q) * CW;
                // the first maximum of the fp32 row, a NaN counting as one (fmap_argmax over the logits)
                int a = 0;
                float best = det_ld(logits, base, bf_lg);
                for (int c = 1; c < CW; ++c) {
                    const float v = det_ld(logits, base + c, bf_lg);
                    if (best == best && (v > best || v != v)) { a = c; best = v; }
                }
                float s = NAN;
                if (best == best) {                     // no NaN in the row: best is its maximum, exp(best - max) = 1
                    float sum = 0.f;
                    for (int c = 0; c < CW; ++c) sum += expf(det_ld(logits, base + c, bf_lg) - best);
                    s = 1.f / sum;
                }
                s_lab[q] = a;
                if (a != C && s == s && s >= score_thr) { key = fmap_key(s, q); ++mine; }
            }
            keys[q] = key;
        }
    }
    // ---- the number of candidates: wave sums, then the waves in order ----
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) mine += __shfl_xor(mine, s, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = mine;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < DET_THREADS / 64; ++w) total += s_cnt[w];
    const int count = total < K ? total : K;

    // ---- bitonic sort of keys[0, n2) descending ----
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += DET_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long x = keys[lo], y = keys[hi];
                const bool desc = (lo & k) == 0;
                if (desc ? x < y : x > y) { keys[lo] = y; keys[hi] = x; }
            }
            __syncthreads();
        }
    }

    // ---- rows [0, count): the ranked detections; rows [count, K): the empty row ----
    const float H = sizes[2 * b], W = sizes[2 * b + 1];
    for (int r = tid; r < K; r += DET_THREADS) {
        const long o = (long)b * K + r;
        float bx[4] = {0.f, 0.f, 0.f, 0.f}, score = 0.f, aux = 0.f;
        int label = -1, query = -1;
        if (r < count) {
            const unsigned long long key = keys[r];
            const int i = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
            score = det_score_of(key);
            if (TOP1) {
                query = i;
                label = s_lab[i];
                aux = lb_rows == 1 ? s_pb[0] : det_prob1(logits_b, qrow0 + i, NB, bf_lb);
            } else {
                query = i / C;
                label = i - query * C;
                aux = s_pb[query];
            }
            const long br = (qrow0 + query) * 4;
            const float cx = det_ld(boxes, br, bf_bx), cy = det_ld(boxes, br + 1, bf_bx), w = det_ld(boxes, br + 2, bf_bx),
                        h = det_ld(boxes, br + 3, bf_bx);
            {
#pragma clang fp contract(off)
                const float hw = 0.5f * w, hh = 0.5f * h;
                const float x1 = cx - hw, y1 = cy - hh, x2 = cx + hw, y2 = cy + hh;
                bx[0] = x1 * W; bx[1] = y1 * H; bx[2] = x2 * W; bx[3] = y2 * H;
            }
        }
        *(f32x4*)(det_box + o * 4) = f32x4{bx[0], bx[1], bx[2], bx[3]};
        det_score[o] = score;
        det_label[o] = label;
        det_query[o] = query;
        det_aux[o] = aux;
    }
    if (tid == 0) {
        det_count[b] = count;
        det_total[b] = total;
    }
}

// Actor decode (AVA rule; detect.decode_actors_host is the definition): the clip's ACTORS -- queries with pb = softmax(logits_b)[1] > actor_thr --
// ranked by pb descending, then query ascending (fmap_key(pb, q) sorted in LDS as above), the best A kept, each with its box and its WHOLE action
// row sigmoid(logit) * pb, unthresholded: det_actions[a][c] is the number detect_kernel<0> calls the score of (query, c), bit for bit.
#define DETA_MAX_QS 1024          // queries of a clip: 8 KB of keys
#define DETA_MAX_A 1024

__global__ __launch_bounds__(DET_THREADS) void detect_actors_kernel(const void* __restrict__ logits, const void* __restrict__ logits_b,
                                                                    const void* __restrict__ boxes, const float* __restrict__ sizes,
                                                                    const int* __restrict__ q_begin, int Qtot, int Qs, int C, int NB, int lb_rows,
                                                                    int dtypes, float actor_thr, int A, float* __restrict__ det_box,
                                                                    float* __restrict__ det_actor, int* __restrict__ det_query,
                                                                    float* __restrict__ det_actions, int* __restrict__ det_count,
                                                                    int* __restrict__ det_total) {
    __shared__ unsigned long long keys[DETA_MAX_QS];
    __shared__ float s_pb[DETA_MAX_QS];
    __shared__ int s_cnt[DET_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool bf_lg = dtypes & DET_BF16_LOGITS, bf_lb = dtypes & DET_BF16_LOGITS_B, bf_bx = dtypes & DET_BF16_BOXES;
    int n2 = 2;
    while (n2 < Qs) n2 <<= 1;                           // <= DETA_MAX_QS (the launcher checked Qs)
    int q0 = q_begin ? q_begin[b] : 0;
    const bool slice_ok = q0 >= 0 && q0 <= Qtot - Qs;   // a slice outside the clip's queries: an empty result, nothing read
    if (!slice_ok) q0 = 0;
    const long qrow0 = (long)b * Qtot + q0;

    // ---- per query: the actor probability and its order key ----
    int mine = 0;
    for (int q = tid; q < n2; q += DET_THREADS) {
        unsigned long long key = 0ull;
        if (q < Qs && slice_ok) {
            const float pb = det_prob1(logits_b, lb_rows == 1 ? (long)b : qrow0 + q, NB, bf_lb);
            s_pb[q] = pb;
            if (pb > actor_thr) { key = fmap_key(pb, q); ++mine; }          // a NaN is no actor
        }
        keys[q] = key;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) mine += __shfl_xor(mine, s, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = mine;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < DET_THREADS / 64; ++w) total += s_cnt[w];
    const int count = total < A ? total : A;

    // ---- bitonic sort of keys[0, n2) descending ----
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += DET_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long x = keys[lo], y = keys[hi];
                const bool desc = (lo & k) == 0;
                if (desc ? x < y : x > y) { keys[lo] = y; keys[hi] = x; }
            }
            __syncthreads();
        }
    }

    // ---- rows [0, count): box, actor probability, query; rows [count, A): the empty row ----
    const float H = sizes[2 * b], W = sizes[2 * b + 1];
    for (int r = tid; r < A; r += DET_THREADS) {
        const long o = (long)b * A + r;
        float bx[4] = {0.f, 0.f, 0.f, 0.f}, actor = 0.f;
        int query = -1;
        if (r < count) {
            const unsigned long long key = keys[r];
            query = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
            actor = det_score_of(key);
            const long br = (qrow0 + query) * 4;
            const float cx = det_ld(boxes, br, bf_bx), cy = det_ld(boxes, br + 1, bf_bx), w = det_ld(boxes, br + 2, bf_bx),
                        h = det_ld(boxes, br + 3, bf_bx);
            {
#pragma clang fp contract(off)
                const float hw = 0.5f * w, hh = 0.5f * h;
                const float x1 = cx - hw, y1 = cy - hh, x2 = cx + hw, y2 = cy + hh;
                bx[0] = x1 * W; bx[1] = y1 * H; bx[2] = x2 * W; bx[3] = y2 * H;
            }
        }
        *(f32x4*)(det_box + o * 4) = f32x4{bx[0], bx[1], bx[2], bx[3]};
        det_actor[o] = actor;
        det_query[o] = query;
    }

    // ---- the action rows [A][C], consecutive threads on consecutive classes; rows behind count are zero ----
    float* __restrict__ act = det_actions + (long)b * A * C;
    if ((C & 3) == 0 && ((uintptr_t)det_actions & 15) == 0) {           // rows of whole 16-byte groups, each aligned
        const int C4 = C >> 2;
        for (int g = tid; g < A * C4; g += DET_THREADS) {
            const int r = g / C4, c0 = (g - r * C4) << 2;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (r < count) {
                const int query = (int)(0xFFFFFFFFu - (unsigned)(keys[r] & 0xFFFFFFFFull));
                const float pb = s_pb[query];
                const long base = (qrow0 + query) * C + c0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = det_ld(logits, base + j, bf_lg);
                    const float s = (1.f / (1.f + expf(-x))) * pb;
                    v[j] = s;
                }
            }
            *(f32x4*)(act + (long)r * C + c0) = f32x4{v[0], v[1], v[2], v[3]};
        }
    } else {
        for (int i = tid; i < A * C; i += DET_THREADS) {
            const int r = i / C, c = i - r * C;
            float v = 0.f;
            if (r < count) {
                const int query = (int)(0xFFFFFFFFu - (unsigned)(keys[r] & 0xFFFFFFFFull));
                const float pb = s_pb[query];
                const float x = det_ld(logits, (qrow0 + query) * C + c, bf_lg);
                const float s = (1.f / (1.f + expf(-x))) * pb;
                v = s;
            }
            act[i] = v;
        }
    }
    if (tid == 0) {
        det_count[b] = count;
        det_total[b] = total;
    }
}

static int detect_check(const void* logits, const void* logits_b, const void* boxes, const float* sizes, int B, int Qtot, int Qs, int C, int NB,
                        int lb_rows, int dtypes, float actor_thr, float score_thr, int K, const void* o0, const void* o1, const void* o2,
                        const void* o3, const void* o4, const void* o5, const void* o6) {
    if (B < 1 || Qtot < 1 || Qs < 1 || Qs > Qtot || C < 1 || K < 1 || NB < 2 || NB > DET_MAX_NB) return TUBER_EINVAL;
    if (lb_rows != 1 && lb_rows != Qtot) return TUBER_EINVAL;
    if (dtypes & ~(DET_BF16_LOGITS | DET_BF16_LOGITS_B | DET_BF16_BOXES)) return TUBER_EINVAL;
    if (!(actor_thr == actor_thr) || !(score_thr == score_thr)) return TUBER_EINVAL;
    if (!logits || !logits_b || !boxes || !sizes || !o0 || !o1 || !o2 || !o3 || !o4 || !o5 || !o6) return TUBER_EINVAL;
    if ((long)Qs * C > DET_MAX_KEYS || K > DET_MAX_K) return DET_EBOUNDS;
    return TUBER_OK;
}

extern "C" {

// AVA rule.  pred_logits [B][Qtot][C], pred_logits_b [B][lb_rows][NB] (lb_rows = Qtot, or 1: one row per clip), pred_boxes [B][Qtot][4] cxcywh in
// (0, 1), each fp32 or bf16 by its bit of `dtypes` (1 logits, 2 logits_b, 4 boxes); sizes [B][2] fp32 (h, w); q_begin DEVICE int[B] (NULL: 0): the
// clip's Qs queries start there (the key frame's slice of a SINGLE_FRAME: False model); a slice outside [0, Qtot] gives that clip an empty result.
// Out: det_box [B][K][4] fp32 xyxy pixels, det_score / det_aux (actor probability) [B][K] fp32, det_label (class) / det_query (query in the slice)
// [B][K] int, rows from det_count[b] = min(det_total[b], K) on: box 0, score 0, aux 0, label -1, query -1; det_total [B] the candidates before the
// cap.  Qs * C > tuber_detect_limits(0) or K > tuber_detect_limits(1): -2, nothing launched, nothing written; bad sizes or pointers: -1.
int tuber_detect_ava(const void* pred_logits, const void* pred_logits_b, const void* pred_boxes, const float* sizes, const int* q_begin, int B,
                     int Qtot, int Qs, int C, int NB, int lb_rows, int dtypes, float actor_thr, float score_thr, int K, float* det_box,
                     float* det_score, int* det_label, int* det_query, float* det_aux, int* det_count, int* det_total, hipStream_t stream) {
    const int rc = detect_check(pred_logits, pred_logits_b, pred_boxes, sizes, B, Qtot, Qs, C, NB, lb_rows, dtypes, actor_thr, score_thr, K, det_box,
                                det_score, det_label, det_query, det_aux, det_count, det_total);
    if (rc != TUBER_OK) return rc;
    hipLaunchKernelGGL(detect_kernel<0>, dim3(B), dim3(DET_THREADS), 0, stream, pred_logits, pred_logits_b, pred_boxes, sizes, q_begin, Qtot, Qs, C,
                       NB, lb_rows, dtypes, actor_thr, score_thr, K, det_box, det_score, det_label, det_query, det_aux, det_count, det_total);
    TUBER_RETURN_LAUNCH();
}

// JHMDB / UCF101-24 rule: pred_logits [B][Qtot][C + 1], the no-object column last; det_aux: the visibility probability softmax(logits_b)[1] of the
// query's row (lb_rows = Qtot) or of the clip (lb_rows = 1, what the model produces); actor_thr is not read.  Everything else as tuber_detect_ava.
int tuber_detect_top1(const void* pred_logits, const void* pred_logits_b, const void* pred_boxes, const float* sizes, const int* q_begin, int B,
                      int Qtot, int Qs, int C, int NB, int lb_rows, int dtypes, float actor_thr, float score_thr, int K, float* det_box,
                      float* det_score, int* det_label, int* det_query, float* det_aux, int* det_count, int* det_total, hipStream_t stream) {
    const int rc = detect_check(pred_logits, pred_logits_b, pred_boxes, sizes, B, Qtot, Qs, C, NB, lb_rows, dtypes, actor_thr, score_thr, K, det_box,
                                det_score, det_label, det_query, det_aux, det_count, det_total);
    if (rc != TUBER_OK) return rc;
    hipLaunchKernelGGL(detect_kernel<1>, dim3(B), dim3(DET_THREADS), 0, stream, pred_logits, pred_logits_b, pred_boxes, sizes, q_begin, Qtot, Qs, C,
                       NB, lb_rows, dtypes, actor_thr, score_thr, K, det_box, det_score, det_label, det_query, det_aux, det_count, det_total);
    TUBER_RETURN_LAUNCH();
}

// the bounds of the two entries: which = 0 the largest Qs * C, 1 the largest K, 2 the largest NB; anything else -1
int tuber_detect_limits(int which) {
    return which == 0 ? DET_MAX_KEYS : which == 1 ? DET_MAX_K : which == 2 ? DET_MAX_NB : -1;
}

// Actor decode, AVA rule (detect.decode_actors_host: the definition).  Inputs as tuber_detect_ava.  An ACTOR is a query of the clip's slice whose
// pb = softmax(pred_logits_b)[1] is not NaN and > actor_thr; the best A by pb descending, then query ascending, are kept.  Out: det_box [B][A][4]
// fp32 xyxy pixels, det_actor [B][A] fp32 (pb), det_query [B][A] int (query in the slice), det_actions [B][A][C] fp32 = sigmoid(logit) * pb for
// EVERY class (bit-identical to tuber_detect_ava's score of the same (query, class); a NaN logit stays NaN), det_count [B] = min(det_total, A),
// det_total [B]; rows from det_count on: box 0, actor 0, query -1, actions 0.  Qs, A or NB beyond tuber_detect_actors_limits, or A * C beyond an
// int32: -2, nothing launched, nothing written; bad sizes or pointers, a NaN threshold: -1.
int tuber_detect_actors(const void* pred_logits, const void* pred_logits_b, const void* pred_boxes, const float* sizes, const int* q_begin, int B,
                        int Qtot, int Qs, int C, int NB, int lb_rows, int dtypes, float actor_thr, int A, float* det_box, float* det_actor,
                        int* det_query, float* det_actions, int* det_count, int* det_total, hipStream_t stream) {
    if (B < 1 || Qtot < 1 || Qs < 1 || Qs > Qtot || C < 1 || A < 1 || NB < 2) return TUBER_EINVAL;
    if (lb_rows != 1 && lb_rows != Qtot) return TUBER_EINVAL;
    if (dtypes & ~(DET_BF16_LOGITS | DET_BF16_LOGITS_B | DET_BF16_BOXES)) return TUBER_EINVAL;
    if (!(actor_thr == actor_thr)) return TUBER_EINVAL;
    if (!pred_logits || !pred_logits_b || !pred_boxes || !sizes || !det_box || !det_actor || !det_query || !det_actions || !det_count || !det_total)
        return TUBER_EINVAL;
    if (((uintptr_t)det_box & 15)) return TUBER_EINVAL;
    if (Qs > DETA_MAX_QS || A > DETA_MAX_A || NB > DET_MAX_NB || (long)A * C > 0x7FFFFFFFl) return DET_EBOUNDS;
    hipLaunchKernelGGL(detect_actors_kernel, dim3(B), dim3(DET_THREADS), 0, stream, pred_logits, pred_logits_b, pred_boxes, sizes, q_begin, Qtot, Qs, C,
                       NB, lb_rows, dtypes, actor_thr, A, det_box, det_actor, det_query, det_actions, det_count, det_total);
    TUBER_RETURN_LAUNCH();
}

// the bounds of tuber_detect_actors: which = 0 the largest Qs, 1 the largest A, 2 the largest NB; anything else -1
int tuber_detect_actors_limits(int which) {
    return which == 0 ? DETA_MAX_QS : which == 1 ? DETA_MAX_A : which == 2 ? DET_MAX_NB : -1;
}

}  // extern "C"
