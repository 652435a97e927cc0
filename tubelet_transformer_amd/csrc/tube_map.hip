// Video-mAP of the JHMDB / UCF101-24 validation loop on the device (gfx950): the two sequential steps behind device_map.DeviceVideoMAP.  They
// restate evaluation.VideoMAP, which is the definition (the reference ships no tube linking and no video-level evaluator).
//   1. tube_rows_kernel     a thread per row: the arg-max column of its C + 1 probabilities (tube_rows_ranked_kernel: the class the caller gives)
//      tube_link_kernel     a wave per (video, class) walks the video's slots in order.  A lane holds one active tube (last box, fp64 score sum,
//                           count, last slot, head) AND one row of the current slot; the visiting order of the tubes is a rank over
//                           (mean score, head), the pick of a tube a wave arg-max over the order keys of the rows it may take.
//                           Its STREAM form (tuber_tube_link_stream, video.VideoStream) links one video whose slots arrive in pieces: the
//                           lanes are loaded from and stored to a caller-owned state around the walk.
//   2. tube_match_kernel    a wave per (video, class) on the slot walk it shares with step 4 (tube_span .. tube_next_head: the live tubes in
//                           lanes, then the counted heads by descending score): adds the per-slot IoU against the ground-truth boxes of the class
//                           into a [64][32] table (tube lane x ground-truth tube), writes a tube's spatio-temporal IoU row when the tube ends, and
//                           matches the visited tubes greedily, a lane per threshold with its taken set in one 32-bit mask.
//   3. track_actions_kernel (tuber_track_actions, actor tracks of an AVA video): behind tube_link_kernel run with one class over a [S][A] actor store, a
//                           workgroup per row averages the action rows of the row's track -- over the whole track at its head, over a window of slots
//                           at every row -- in fp64, sequentially in slot order.
//   4. tube_nms_kernel      (tuber_tube_nms, evaluation.tube_nms: the definition) between steps 1 and 2, or behind step 1 over a padded store: step
//                           2's walk with a [64][64] table of the per-slot IoU of every two live tubes; the pairs above the threshold are recorded
//                           when the first of the two ends, and a visited tube is suppressed iff a kept one overlaps.
//   5. tube_dense_kernel    (tuber_tube_dense, evaluation.dense_rows: the definition) behind step 1 (and step 4) over a padded store: a wave per row
//                           finds the row's successor by one ballot and writes a box and a score for every frame up to it.
// No floating-point atomics, every sum sequential in slot order: the same input gives the same bits.
#include "map_common.h"

#define TUBE_MAX_ACTIVE 64        // simultaneously active tubes of one (video, class): a lane each
#define TUBE_MAX_GT 32            // ground-truth tubes of one (video, class): the taken set is one 32-bit mask
#define TUBE_MAX_THR 16           // thresholds of one call
#define TUBE_NOT_COUNTED 2
#define TUBE_BEYOND_BOUNDS 3
#define TLINK_WAVES 4             // (video, class) pairs per workgroup of the link kernel: a wave each
#define TMATCH_LD 33              // leading dimension of the LDS tables of the match kernel

__device__ __forceinline__ unsigned long long tube_wave_max(unsigned long long k) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_xor(k, o, 64);
        k = t > k ? t : k;
    }
    return k;
}

// a double as an order-preserving unsigned (-0 == +0, NaN below everything)
__device__ __forceinline__ unsigned long long tube_ord(double s) {
    unsigned long long u = (unsigned long long)__double_as_longlong(s);
    if (s != s) return 0ull;
    if (s == 0.0) u = 0ull;
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void tube_rows_kernel(const float* __restrict__ det_prob, int N, int C, int* __restrict__ row_cls,
                                                        int* __restrict__ row_head) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    float score;
    row_cls[r] = fmap_argmax(det_prob + (long)r * (C + 1), C, score);
    row_head[r] = -1;
}

// the ranked form (tuber_tube_link_ranked): a row's class is what the caller gives, C where that is no class of the call
__global__ __launch_bounds__(256) void tube_rows_ranked_kernel(const int* __restrict__ det_label, int N, int C, int* __restrict__ row_cls,
                                                               int* __restrict__ row_head) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int l = det_label[r];
    row_cls[r] = (l >= 0 && l < C) ? l : C;
    row_head[r] = -1;
}

// the linker's state of one video between two tuber_tube_link_stream calls: per (class, lane) what a lane of tube_link_kernel holds, in plain
// arrays of C * 64 entries one behind the other (all zero: no tubes)
struct TubeLinkState {
    double* sum;
    float4* box;
    int *valid, *cnt, *last, *head;
    __host__ __device__ TubeLinkState(unsigned char* p, long lanes)
        : sum((double*)p), box((float4*)(p + 8 * lanes)), valid((int*)(p + 24 * lanes)), cnt((int*)(p + 28 * lanes)), last((int*)(p + 32 * lanes)),
          head((int*)(p + 36 * lanes)) {}
};
#define TUBE_STATE_LANE_BYTES 40

// RANKED: det_prob is det_score [N], a row's score; otherwise [N][C + 1], the score being the wave's column of the row.
// STREAM (tuber_tube_link_stream): ONE video whose S slots of K rows each carry the ordinals slot_base .. slot_base + S - 1; the lanes are loaded
// from `state` and stored back to it; row_cls is det_label; a head is the global row ordinal * K + position; tube_score / tube_len are PER ROW
// (the tube's mean and count after taking the row) and tube_last is not written.
template <bool RANKED, bool STREAM>
__global__ __launch_bounds__(64 * TLINK_WAVES) void tube_link_kernel(const float* __restrict__ det_box, const float* __restrict__ det_prob,
                                                                     const int* __restrict__ slot_off, const int* __restrict__ video_off, int V,
                                                                     int S, int N, int C, double link_iou, int max_gap,
                                                                     const int* __restrict__ row_cls, int* __restrict__ row_head,
                                                                     double* __restrict__ tube_score, int* __restrict__ tube_len,
                                                                     int* __restrict__ tube_last, int K, int slot_base,
                                                                     unsigned char* __restrict__ state) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * TLINK_WAVES + (threadIdx.x >> 6);           // wave-uniform from here on
    if (w >= (long)V * C) return;
    const int v = (int)(w / C), c = (int)(w % C);
    const int s0 = STREAM ? 0 : video_off[v], s1 = STREAM ? S : video_off[v + 1];
    if (s0 < 0 || s1 < s0 || s1 > S) return;                                      // not a CSR row of these arrays: touch nothing
    const int hbase = STREAM ? slot_base * K : 0;                                 // global row of this call's row 0
    const int limit = max_gap + 1 > TUBE_MAX_ACTIVE ? 0 : TUBE_MAX_ACTIVE / (max_gap + 1);
    // the tube this lane holds
    bool valid = false;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
    double sum = 0.0;
    int cnt = 0, last = 0, head = 0;
    const TubeLinkState st(state, (long)C * 64);
    if (STREAM) {
        const int i = c * 64 + lane;
        const float4 b = st.box[i];
        valid = st.valid[i] != 0;
        t0 = b.x; t1 = b.y; t2 = b.z; t3 = b.w;
        sum = st.sum[i]; cnt = st.cnt[i]; last = st.last[i]; head = st.head[i];
    }
    for (int sl = s0; sl < s1; ++sl) {
        const int s = STREAM ? slot_base + sl : sl;                               // the slot's ordinal in its video's numbering
        const int r0 = STREAM ? sl * K : slot_off[sl], r1 = STREAM ? r0 + K : slot_off[sl + 1];
        if (r0 < 0 || r1 < r0 || r1 > N) return;
        const int n = r1 - r0;
        if (n > limit) return;                                                    // the caller's bookkeeping should have kept this video away
        if (n == 0) continue;
        // the row this lane holds: counted rows of the wave's class
        const int r = r0 + lane;
        bool mine = false;
        float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, sc = 0.f;
        if (lane < n && row_cls[r] == c) {
            const float* d = det_box + (long)r * 4;
            b0 = d[0]; b1 = d[1]; b2 = d[2]; b3 = d[3];
            sc = RANKED ? det_prob[r] : det_prob[(long)r * (C + 1) + c];
            mine = b0 < b2 && b1 < b3 && sc == sc;
        }
        if (!__ballot(mine)) continue;
        // the active tubes in visiting order: rank = tubes in front of this one (mean score descending, then head ascending)
        const bool active = valid && s - last <= max_gap + 1;
        const unsigned long long amask = __ballot(active);
        const double mean = active ? sum / (double)cnt : 0.0;
        int rank = 0;
        for (unsigned long long m = amask; m; m &= m - 1) {
            const int j = __ffsll((long long)m) - 1;
            const double mj = __shfl(mean, j, 64);
            const int hj = __shfl(head, j, 64);
            rank += (mj > mean || (mj == mean && hj < head)) ? 1 : 0;
        }
        const int na = __popcll(amask);
        bool claimed = false;
        for (int k = 0; k < na; ++k) {
            const unsigned long long tm = __ballot(active && rank == k);
            if (!tm) continue;
            const int t = __ffsll((long long)tm) - 1;
            const float l0 = __shfl(t0, t, 64), l1 = __shfl(t1, t, 64), l2 = __shfl(t2, t, 64), l3 = __shfl(t3, t, 64);
            const double iou = fmap_iou_d((double)l0, (double)l1, (double)l2, (double)l3, (double)b0, (double)b1, (double)b2, (double)b3);
            const bool elig = mine && !claimed && iou >= link_iou;
            const unsigned long long best = tube_wave_max(elig ? fmap_key(sc, lane) : 0ull);   // a key is > 0: its low word is >= ~63
            if (!best) continue;
            const int p = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
            const float n0 = __shfl(b0, p, 64), n1 = __shfl(b1, p, 64), n2 = __shfl(b2, p, 64), n3 = __shfl(b3, p, 64);
            const float ns = __shfl(sc, p, 64);
            const int ht = __shfl(head, t, 64);
            if (lane == p) {
                claimed = true;
                row_head[r] = ht;
            }
            if (lane == t) {
                t0 = n0; t1 = n1; t2 = n2; t3 = n3;
                sum += (double)ns;
                cnt += 1;
                last = s;
                const int at = STREAM ? r0 + p : head;
                tube_score[at] = sum / (double)cnt;
                tube_len[at] = cnt;
                if (!STREAM) tube_last[head] = s;
            }
        }
        // the rows nobody took start tubes, in the lanes of tubes that cannot be active at the next slot
        unsigned long long um = __ballot(mine && !claimed);
        unsigned long long fm = __ballot(!valid || s - last > max_gap);
        for (; um; um &= um - 1) {
            if (!fm) return;                                                      // cannot happen within the bounds the launcher checks
            const int p = __ffsll((long long)um) - 1;
            const int t = __ffsll((long long)fm) - 1;
            fm &= fm - 1;
            const float n0 = __shfl(b0, p, 64), n1 = __shfl(b1, p, 64), n2 = __shfl(b2, p, 64), n3 = __shfl(b3, p, 64);
            const float ns = __shfl(sc, p, 64);
            if (lane == p) row_head[r] = hbase + r;
            if (lane == t) {
                valid = true;
                t0 = n0; t1 = n1; t2 = n2; t3 = n3;
                sum = (double)ns;
                cnt = 1;
                last = s;
                head = hbase + r0 + p;
                const int at = STREAM ? r0 + p : head;
                tube_score[at] = sum;
                tube_len[at] = 1;
                if (!STREAM) tube_last[head] = s;
            }
        }
    }
    if (STREAM) {
        const int i = c * 64 + lane;
        st.box[i] = make_float4(t0, t1, t2, t3);
        st.valid[i] = valid ? 1 : 0;
        st.sum[i] = sum; st.cnt[i] = cnt; st.last[i] = last; st.head[i] = head;
    }
}

// every row of a tuber_tube_link_stream call starts as "not counted"
__global__ __launch_bounds__(256) void tube_rows_stream_kernel(int N, int* __restrict__ row_head, double* __restrict__ row_score,
                                                               int* __restrict__ row_len) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    row_head[r] = -1;
    row_score[r] = 0.0;
    row_len[r] = 0;
}

// The slot walk of tube_match_kernel and tube_nms_kernel, a workgroup of ONE wave per (video, class).  Phase 1 walks the video's slots in order:
// a lane holds one row of the current slot AND one live tube (head, tube_last, tube_len), whose sums sit in the LDS table row of the lane.
// Phase 2 visits the class's counted heads by descending score.  The helpers with a ballot or a shuffle are reached by all 64 lanes.

// the slots [s0, s1) and the rows [R0, R1) of video v; false: not a CSR row of these arrays, touch nothing
__device__ __forceinline__ bool tube_span(const int* __restrict__ video_off, const int* __restrict__ slot_off, int v, int S, int N, int& s0, int& s1,
                                          int& R0, int& R1) {
    s0 = video_off[v]; s1 = video_off[v + 1];
    if (s0 < 0 || s1 < s0 || s1 > S) return false;
    R0 = slot_off[s0]; R1 = slot_off[s1];
    return !(R0 < 0 || R1 < R0 || R1 > N);
}

// the row r of a slot of n rows that this lane holds: its head and box, -1 without a row of class c.  A head is a head row of class c in
// [R0, r] (the linkers write no other), so the `work` row of a head is this wave's whatever the record holds.
__device__ __forceinline__ int tube_slot_row(const float* __restrict__ det_box, const int* __restrict__ row_cls, const int* __restrict__ row_head,
                                             int r, int lane, int n, int c, int R0, float& b0, float& b1, float& b2, float& b3) {
    int rh = -1;
    b0 = b1 = b2 = b3 = 0.f;
    if (lane < n && row_cls[r] == c) {                                            // behind the class two memory round trips: head and box, then the
        const float* d = det_box + (long)r * 4;                                   // head's row; no branch in between that would chain the loads
        const int h = row_head[r];
        const float d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
        const int hr = h >= R0 && h <= r ? h : r;                                 // a row in bounds whatever h is
        const bool ok = (hr == h) & (row_cls[hr] == c) & (row_head[hr] == hr);
        rh = ok ? h : -1;
        b0 = ok ? d0 : 0.f; b1 = ok ? d1 : 0.f; b2 = ok ? d2 : 0.f; b3 = ok ? d3 : 0.f;
    }
    return rh;
}

// the lane that holds the live tube of head h (wave-uniform); without one the first free lane, `begins` set: the kernel fills the lane and
// zeroes its tables; -1 when every lane is taken: the (video, class) is beyond the bounds
__device__ __forceinline__ int tube_lane_of(bool valid, int head, int h, bool& begins) {
    const unsigned long long tm = __ballot(valid && head == h);
    begins = !tm;
    if (tm) return __ffsll((long long)tm) - 1;
    const unsigned long long fm = ~__ballot(valid);
    return fm ? __ffsll((long long)fm) - 1 : -1;
}

// nothing is decided for a (video, class) beyond the bounds: byte 3 at its heads, in each of the `planes` N-strided planes of `flag`
__device__ __forceinline__ void tube_mark_beyond(const int* __restrict__ row_cls, const int* __restrict__ row_head, int R0, int R1, int c, int lane,
                                                 unsigned char* __restrict__ flag, int planes, int N) {
    for (int r = R0 + lane; r < R1; r += 64)
        if (row_cls[r] == c && row_head[r] == r)
            for (int i = 0; i < planes; ++i) flag[(long)i * N + r] = TUBE_BEYOND_BOUNDS;
}

// phase 2's visiting order: the heads of class c in [R0, R1) with tube_len >= min_len by descending tube_ord(score), equal scores by ascending
// head.  (last_hi, last_lo) is the key of the head visited last, (~0, ~0) before the first one; -> the next head (wave-uniform), -1: done
__device__ __forceinline__ int tube_next_head(const int* __restrict__ row_cls, const int* __restrict__ row_head, const double* __restrict__ tube_score,
                                              const int* __restrict__ tube_len, int R0, int R1, int c, int min_len, int lane,
                                              unsigned long long& last_hi, unsigned long long& last_lo) {
    unsigned long long best_hi = 0ull, best_lo = 0ull;                            // a real key has lo > 0
    for (int r = R0 + lane; r < R1; r += 64) {
        if (row_cls[r] != c || row_head[r] != r || tube_len[r] < min_len) continue;
        const unsigned long long hi = tube_ord(tube_score[r]), lo = 0xFFFFFFFFull - (unsigned long long)(r - R0);
        if (!(hi < last_hi || (hi == last_hi && lo < last_lo))) continue;
        if (hi > best_hi || (hi == best_hi && lo > best_lo)) { best_hi = hi; best_lo = lo; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long oh = __shfl_xor(best_hi, o, 64), ol = __shfl_xor(best_lo, o, 64);
        if (oh > best_hi || (oh == best_hi && ol > best_lo)) { best_hi = oh; best_lo = ol; }
    }
    if (!best_lo) return -1;
    last_hi = best_hi; last_lo = best_lo;
    return R0 + (int)(0xFFFFFFFFull - best_lo);
}

__global__ __launch_bounds__(64) void tube_match_kernel(const float* __restrict__ det_box, const int* __restrict__ slot_off,
                                                        const int* __restrict__ video_off, const int* __restrict__ row_cls,
                                                        const int* __restrict__ row_head, const double* __restrict__ tube_score,
                                                        const int* __restrict__ tube_len, const int* __restrict__ tube_last,
                                                        const double* __restrict__ gt_box, const int* __restrict__ gt_cls,
                                                        const int* __restrict__ gt_tube, const int* __restrict__ gt_off,
                                                        const double* __restrict__ thresholds, int S, int N, int G, int C, int T, int K, int min_len,
                                                        double* __restrict__ work, unsigned char* __restrict__ tube_flag) {
    __shared__ double s_acc[TUBE_MAX_ACTIVE * TMATCH_LD];                         // [tube lane][ground-truth tube]: sum of the per-slot IoU
    __shared__ int s_cnt[TUBE_MAX_ACTIVE * TMATCH_LD];                            // slots the two share
    __shared__ int s_glen[TUBE_MAX_GT];                                           // slots of a ground-truth tube; 0: no such tube
    const int lane = threadIdx.x;
    const int v = blockIdx.x / C, c = blockIdx.x % C;
    int s0, s1, R0, R1;
    if (!tube_span(video_off, slot_off, v, S, N, s0, s1, R0, R1)) return;
    const int G0 = gt_off[s0], G1 = gt_off[s1];
    if (G0 < 0 || G1 < G0 || G1 > G) return;
    const int KS = K > 0 ? K : 1;
    if (lane < TUBE_MAX_GT) s_glen[lane] = 0;
    __syncthreads();
    for (int i = G0 + lane; i < G1; i += 64) {
        const int k = gt_tube[i];
        if (gt_cls[i] == c && k >= 0 && k < K) atomicAdd(&s_glen[k], 1);          // integers: any order
    }
    __syncthreads();

    // phase 1: the spatio-temporal IoU of every tube of the class with every ground-truth tube of the class
    bool valid = false, beyond = false;
    int head = -1, last = -1, len = 0;
    for (int s = s0; s < s1 && !beyond; ++s) {
        const int r0 = slot_off[s], r1 = slot_off[s + 1], g0 = gt_off[s], g1 = gt_off[s + 1];
        if (r0 < R0 || r1 < r0 || r1 > R1 || g0 < G0 || g1 < g0 || g1 > G1) return;
        const int n = r1 - r0, g = g1 - g0;
        if (n > FMAP_MAX_DETS || g > FMAP_MAX_GT) { beyond = true; break; }
        float b0, b1, b2, b3;
        const int rh = tube_slot_row(det_box, row_cls, row_head, r0 + lane, lane, n, c, R0, b0, b1, b2, b3);
        int gk = -1;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
        if (lane < g && gt_cls[g0 + lane] == c) {
            const int k = gt_tube[g0 + lane];
            if (k >= 0 && k < K) {
                const double* q = gt_box + (long)(g0 + lane) * 4;
                gk = k; q0 = q[0]; q1 = q[1]; q2 = q[2]; q3 = q[3];
            }
        }
        for (unsigned long long m = __ballot(rh >= 0); m; m &= m - 1) {
            const int p = __ffsll((long long)m) - 1;
            const int h = __shfl(rh, p, 64);
            bool begins;
            const int t = tube_lane_of(valid, head, h, begins);
            if (t < 0) { beyond = true; break; }
            if (begins) {                                                         // its table row zeroed
                if (lane == t) {
                    valid = true;
                    head = h;
                    last = tube_last[h];
                    len = tube_len[h];
                }
                if (lane < TUBE_MAX_GT) {
                    s_acc[t * TMATCH_LD + lane] = 0.0;
                    s_cnt[t * TMATCH_LD + lane] = 0;
                }
                __syncthreads();
            }
            const float p0 = __shfl(b0, p, 64), p1 = __shfl(b1, p, 64), p2 = __shfl(b2, p, 64), p3 = __shfl(b3, p, 64);
            if (gk >= 0) {
                s_acc[t * TMATCH_LD + gk] += fmap_iou_d((double)p0, (double)p1, (double)p2, (double)p3, q0, q1, q2, q3);
                s_cnt[t * TMATCH_LD + gk] += 1;
            }
        }
        if (beyond) break;
        __syncthreads();
        if (valid && last <= s) {                                                 // the tube ends here: its row of the overlap table
            for (int k = 0; k < K; ++k) {
                const int shared = s_cnt[lane * TMATCH_LD + k];
                work[(long)head * KS + k] = shared > 0 ? s_acc[lane * TMATCH_LD + k] / (double)(len + s_glen[k] - shared) : 0.0;
            }
            valid = false;
        }
        __syncthreads();
    }
    if (beyond) return tube_mark_beyond(row_cls, row_head, R0, R1, c, lane, tube_flag, T, N);
    __threadfence();
    __syncthreads();

    // phase 2: a lane per threshold
    const double thr = lane < T ? thresholds[lane] : 0.0;
    unsigned taken = 0u;
    unsigned long long last_hi = ~0ull, last_lo = ~0ull;
    for (int h; (h = tube_next_head(row_cls, row_head, tube_score, tube_len, R0, R1, c, min_len, lane, last_hi, last_lo)) >= 0;) {
        if (lane < T) {
            int bk = -1;                                                          // the largest overlap among the tubes not taken, the first one
            double bv = 0.0;
            for (int k = 0; k < K; ++k) {
                if (s_glen[k] <= 0 || ((taken >> k) & 1u)) continue;
                // read at device scope: the row was written by another lane of this wave, and a neighbouring workgroup on this CU may have
                // pulled the cache line into the vector L1 before that
                const double x = __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)(work + (long)h * KS + k),
                                                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if (bk < 0 || x > bv) { bk = k; bv = x; }
            }
            const bool tp = bk >= 0 && bv >= thr;
            if (tp) taken |= 1u << bk;
            tube_flag[(long)lane * N + h] = tp ? 1 : 0;
        }
    }
}

// Spatio-temporal NMS over the linked tubes (evaluation.tube_nms: the definition; tuber_tube_nms): the slot walk above, tube against tube.
// Phase 1 adds, per slot, the fp64 IoU of every two rows of the class into a [64][64] table (tube lane x tube lane; a row's lane writes only
// its own table row); when a tube ends, every pair it forms with a tube that is still live is final, and its lane writes the heads of the
// partners whose stIoU is above nms_iou into its 64-entry row of `work`.  A pair is thus recorded in the row of the tube that ends first, or
// in both rows.  Phase 2: a visited tube is suppressed iff a kept tube marked it or a partner in its own row is kept; a kept tube marks the
// partners in its row.  The status words (2 not visited, 1 kept, 0 suppressed or marked) follow the partner rows in `work`.
#define TNMS_LD 65                // leading dimension of the LDS tables: a lane reads its own row without bank conflicts
#define TNMS_ROW 64               // partner entries per tube in `work`

__device__ __forceinline__ int tnms_get(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tnms_put(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(64) void tube_nms_kernel(const float* __restrict__ det_box, const int* __restrict__ slot_off,
                                                      const int* __restrict__ video_off, const int* __restrict__ row_cls,
                                                      const int* __restrict__ row_head, const double* __restrict__ tube_score,
                                                      const int* __restrict__ tube_len, const int* __restrict__ tube_last, int S, int N, int C,
                                                      int min_len, double nms_iou, int* __restrict__ work, unsigned char* __restrict__ tube_keep) {
    __shared__ double s_acc[TUBE_MAX_ACTIVE * TNMS_LD];                           // [tube lane][tube lane]: sum of the per-slot IoU
    __shared__ int s_cnt[TUBE_MAX_ACTIVE * TNMS_LD];                              // slots the two share
    __shared__ int s_head[TUBE_MAX_ACTIVE], s_len[TUBE_MAX_ACTIVE];               // the tube a lane holds
    const int lane = threadIdx.x;
    const int v = blockIdx.x / C, c = blockIdx.x % C;
    int s0, s1, R0, R1;
    if (!tube_span(video_off, slot_off, v, S, N, s0, s1, R0, R1)) return;
    int* status = work + (long)N * TNMS_ROW;

    // phase 1: the partners of every tube of the class
    bool valid = false, beyond = false;
    int head = -1, last = -1, len = 0, seen = -1;
    for (int s = s0; s < s1 && !beyond; ++s) {
        const int r0 = slot_off[s], r1 = slot_off[s + 1];
        if (r0 < R0 || r1 < r0 || r1 > R1) return;
        const int n = r1 - r0;
        if (n > FMAP_MAX_DETS) { beyond = true; break; }
        float b0, b1, b2, b3;
        const int rh = tube_slot_row(det_box, row_cls, row_head, r0 + lane, lane, n, c, R0, b0, b1, b2, b3);
        int mine = -1;                                                            // the lane that holds the row's tube
        for (unsigned long long m = __ballot(rh >= 0); m; m &= m - 1) {
            const int p = __ffsll((long long)m) - 1;
            const int h = __shfl(rh, p, 64);
            bool begins;
            const int t = tube_lane_of(valid, head, h, begins);
            if (t < 0) { beyond = true; break; }
            if (!begins && __shfl(seen, t, 64) == s) continue;                    // a second row of one tube in one slot: the first one counts
            if (begins) {                                                         // its table row and column zeroed
                if (lane == t) {
                    valid = true;
                    head = h;
                    last = tube_last[h];
                    last = last > s1 - 1 ? s1 - 1 : last;
                    len = tube_len[h];
                    s_head[t] = h;
                    s_len[t] = len;
                }
                s_acc[t * TNMS_LD + lane] = 0.0;
                s_cnt[t * TNMS_LD + lane] = 0;
                s_acc[lane * TNMS_LD + t] = 0.0;
                s_cnt[lane * TNMS_LD + t] = 0;
                work[(long)h * TNMS_ROW + lane] = -1;
                if (lane == 0) status[h] = 2;
                __syncthreads();
            }
            if (lane == t) seen = s;
            if (lane == p) mine = t;
        }
        if (beyond) break;
        const unsigned long long rows = __ballot(mine >= 0);
        for (unsigned long long m = rows; m; m &= m - 1) {                        // every row against every other row of the slot
            const int p = __ffsll((long long)m) - 1;
            const int tp = __shfl(mine, p, 64);
            const float p0 = __shfl(b0, p, 64), p1 = __shfl(b1, p, 64), p2 = __shfl(b2, p, 64), p3 = __shfl(b3, p, 64);
            if (mine >= 0 && lane != p) {
                s_acc[mine * TNMS_LD + tp] += fmap_iou_d((double)b0, (double)b1, (double)b2, (double)b3, (double)p0, (double)p1, (double)p2, (double)p3);
                s_cnt[mine * TNMS_LD + tp] += 1;
            }
        }
        __syncthreads();
        const unsigned long long live = __ballot(valid);
        if (valid && last <= s) {                                                 // the tube ends here: its pairs with the live tubes are final
            if (len >= min_len) {
                for (unsigned long long m = live & ~(1ull << lane); m; m &= m - 1) {
                    const int j = __ffsll((long long)m) - 1;
                    const int shared = s_cnt[lane * TNMS_LD + j];
                    if (shared <= 0 || s_len[j] < min_len) continue;
                    if (s_acc[lane * TNMS_LD + j] / (double)(len + s_len[j] - shared) > nms_iou) work[(long)head * TNMS_ROW + j] = s_head[j];
                }
            }
            valid = false;
        }
        __syncthreads();
    }
    if (beyond) return tube_mark_beyond(row_cls, row_head, R0, R1, c, lane, tube_keep, 1, N);
    __threadfence();
    __syncthreads();

    // phase 2
    unsigned long long last_hi = ~0ull, last_lo = ~0ull;
    for (int h; (h = tube_next_head(row_cls, row_head, tube_score, tube_len, R0, R1, c, min_len, lane, last_hi, last_lo)) >= 0;) {
        // read at device scope: the words were written by other lanes of this wave, and a neighbouring workgroup on this CU may have pulled
        // their cache lines into the vector L1 before that (tube_match_kernel's work rows)
        const int p = tnms_get(work + (long)h * TNMS_ROW + lane);
        const bool partner = p >= R0 && p < R1;
        const bool hit = partner && tnms_get(status + p) == 1;
        const bool suppressed = tnms_get(status + h) == 0 || __ballot(hit) != 0ull;
        if (!suppressed && partner) tnms_put(status + p, 0);                    // p is not kept, or this tube would be suppressed
        if (lane == 0) {
            tnms_put(status + h, suppressed ? 0 : 1);
            tube_keep[h] = suppressed ? 0 : 1;
        }
        __threadfence();
        __syncthreads();
    }
}

// Dense tubes (evaluation.dense_rows: the definition; tuber_tube_dense): a box and a score on every frame between two linked key detections
// of ONE video's padded [S][K] store.  A wave per row r of slot s.  Phase 1: lane c < K * (max_gap + 1) reads the head of candidate row
// (s + 1 + c / K) * K + c % K -- the slots the linker may have bridged to, in row order -- and the lowest lane of the ballot "my row's head"
// is the successor.  Phase 2: the two boxes, the two scores and g = slot_frame[successor's slot] - slot_frame[s] (1 without a successor) are
// wave-uniform; lane j, j + 64, ... < g writes frame j of the row: the row's own bytes at j = 0, behind that the fp64 interpolation, every
// operation rounded on its own as numpy rounds it.  No LDS, no atomics, plain vector stores; nothing is written at j >= g.
#define TDENSE_WAVES 4            // rows per workgroup: a wave each

__device__ __forceinline__ float tdense_lerp(float a, float b, double w) {
#pragma clang fp contract(off)
    const double d = (double)b - (double)a;
    const double p = d * w;
    const float v = (float)((double)a + p);
    return v != v ? __int_as_float(0x7FC00000) : v;                               // one NaN: the definition's
}

__global__ __launch_bounds__(64 * TDENSE_WAVES) void tube_dense_kernel(const float* __restrict__ det_box, const float* __restrict__ det_score,
                                                                       const int* __restrict__ row_head, const int* __restrict__ slot_frame, int S,
                                                                       int K, int max_gap, int G, float* __restrict__ dense_box,
                                                                       float* __restrict__ dense_score, int* __restrict__ row_span,
                                                                       int* __restrict__ row_next) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * TDENSE_WAVES + (threadIdx.x >> 6);          // wave-uniform from here on
    if (r >= (long)S * K) return;
    const int s = (int)(r / K);
    const int h = row_head[r];
    if (h < 0) {                                                                  // not counted: owns no frame
        if (lane == 0) {
            row_span[r] = 0;
            row_next[r] = -1;
        }
        return;
    }
    // phase 1: the successor
    const int cs = s + 1 + lane / K;
    const bool cand = lane < K * (max_gap + 1) && cs < S;
    const unsigned long long m = __ballot(cand && row_head[(long)cs * K + lane % K] == h);
    int nx = -1;
    long g = 1;
    if (m) {
        const int p = __ffsll((long long)m) - 1;
        const int ns = s + 1 + p / K;
        nx = ns * K + p % K;
        g = (long)slot_frame[ns] - (long)slot_frame[s];
    }
    if (g < 1 || g > G) {                                                         // unsorted slot_frame or a G too small: the host answers
        if (lane == 0) row_span[r] = -1;
        return;
    }
    // phase 2: the frames the row owns
    const float4 a = ((const float4*)det_box)[r];
    const float4 b = nx >= 0 ? ((const float4*)det_box)[nx] : a;
    const float sa = det_score[r];
    const float sb = nx >= 0 ? det_score[nx] : sa;
    float4* ob = (float4*)dense_box + r * G;
    float* os = dense_score + r * G;
    for (int j = lane; j < (int)g; j += 64) {
        float4 v = a;
        float sv = sa;
        if (j > 0) {
            const double w = (double)j / (double)g;
            v.x = tdense_lerp(a.x, b.x, w);
            v.y = tdense_lerp(a.y, b.y, w);
            v.z = tdense_lerp(a.z, b.z, w);
            v.w = tdense_lerp(a.w, b.w, w);
            sv = tdense_lerp(sa, sb, w);
        }
        ob[j] = v;
        os[j] = sv;
    }
    if (lane == 0) {
        row_span[r] = (int)g;
        row_next[r] = nx;
    }
}

// Actor tracks (evaluation.actor_tracks: the definition): per-track and temporally smoothed action scores over ONE video's [S][A] actor store
// linked class-agnostically by tube_link_kernel.  A workgroup per row r = slot * A + a, a wave per 64 classes; a row's track is the rows with its
// row_head, at most one per slot, found by comparing the slot's A heads in the lanes of the wave (one ballot).  Every sum is fp64, sequential in
// slot order, followed by one division: the numpy definition's bits.
#define TRACK_THREADS 256
#define TRACK_MAX_C 4096          // classes of an action row

// the position, in the slot whose A heads are `heads`, of the row whose head is h; -1 when the slot has none (wave-uniform; both track kernels)
__device__ __forceinline__ int tube_member(const int* heads, int A, int h, int lane) {
    const unsigned long long m = __ballot(lane < A && heads[lane] == h);
    return m ? __ffsll((long long)m) - 1 : -1;
}

__global__ __launch_bounds__(TRACK_THREADS) void track_actions_kernel(const float* __restrict__ actions, const int* __restrict__ row_head,
                                                                      const int* __restrict__ tube_last, int S, int A, int C, int window,
                                                                      double* __restrict__ row_smooth, double* __restrict__ track_mean,
                                                                      float* __restrict__ track_peak) {
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = r / A;
    int h = row_head[r];
    if (h < 0 || h > r) h = -1;                                                   // a head is its track's first row
    const bool is_head = h == r;
    const int lo = window >= s ? 0 : s - window;
    const int hi = window >= S - 1 - s ? S - 1 : s + window;
    int last = s;
    if (is_head) {
        last = tube_last[r];
        last = last < s ? s : (last > S - 1 ? S - 1 : last);
    }
    for (int c0 = wave * 64; c0 < C; c0 += TRACK_THREADS) {                       // wave-uniform: every lane takes part in the ballots
        const int c = c0 + lane;
        const bool live = c < C;
        double smooth = 0.0, mean = 0.0;
        float peak = 0.f;
        if (h >= 0) {
            double sum = 0.0;
            int n = 0;
            for (int t = lo; t <= hi; ++t) {
                const int a = tube_member(row_head + t * A, A, h, lane);
                if (a < 0) continue;
                ++n;
                if (live) sum += (double)actions[((long)t * A + a) * C + c];
            }
            smooth = sum / (double)n;                                             // n >= 1: the row itself
            if (is_head) {
                double tot = 0.0;
                int len = 0;
                for (int t = s; t <= last; ++t) {
                    const int a = tube_member(row_head + t * A, A, h, lane);
                    if (a < 0) continue;
                    ++len;
                    if (live) {
                        const float v = actions[((long)t * A + a) * C + c];
                        tot += (double)v;
                        if (len == 1) peak = v;
                        else if (peak == peak && (v != v || v > peak)) peak = v;  // np.max: a NaN stays
                    }
                }
                mean = tot / (double)len;
            }
        }
        if (live) {
            const long o = (long)r * C + c;
            row_smooth[o] = smooth;
            track_mean[o] = mean;
            track_peak[o] = peak;
        }
    }
}

// Actor tracks of a video whose key frames arrive in pieces (evaluation.ActorTracker: the definition; tuber_track_actions_stream).  Given the
// heads every class is independent: a workgroup is ONE wave that owns 64 class columns, a lane per column, and walks the S new slots in order.
// Between calls it keeps the last H = max(2 * window, max_gap + 1) + 1 slots in a caller-owned ring, entry ordinal % H: per row the head and the
// count, per (row, class) the running fp64 sum, the fp32 peak and the fp32 action value.  The ring is laid out PER WAVE -- its own copy of the
// head / count records in front of its own class columns -- so no workgroup reads what another one writes: the entry of slot s overwrites that
// of slot s - H while a neighbouring wave may still be looking rows up in it, and with one copy each that cannot matter.  Inside a wave a
// column is read and written by its own lane only; the head / count records live in LDS during the walk (barriers of one wave), are loaded
// from the ring before it and stored slot by slot.
#define TSTREAM_MAX_WINDOW 31                        // 2 * 31 + 1 = 63 ring slots
#define TSTREAM_MAX_ENTRIES (64 * 63)                // H * A: A * (max_gap + 2) <= 128 and A * (2 * window + 1) <= 64 * 63
#define TSTREAM_COLS 64                              // class columns of a wave

__host__ __device__ inline int tstream_slots(int max_gap, int window) {
    return (2 * window > max_gap + 1 ? 2 * window : max_gap + 1) + 1;
}
// bytes of the head + count records of one wave (16-byte multiple), and of one wave's whole ring
__host__ __device__ inline long tstream_record_bytes(int entries) { return ((long)entries * 8 + 15) & ~15l; }
__host__ __device__ inline long tstream_wave_bytes(int entries) {
    return tstream_record_bytes(entries) + (long)entries * TSTREAM_COLS * 16;
}

__global__ __launch_bounds__(64) void track_actions_stream_kernel(const float* __restrict__ actions, const int* __restrict__ row_head, int S,
                                                                  int A, int C, int slot_base, int max_gap, int window, int flush, int H,
                                                                  unsigned char* __restrict__ state, double* __restrict__ row_mean,
                                                                  float* __restrict__ row_peak, double* __restrict__ smooth) {
    __shared__ int s_head[TSTREAM_MAX_ENTRIES];
    __shared__ int s_cnt[TSTREAM_MAX_ENTRIES];
    const int lane = threadIdx.x;
    const int c = blockIdx.x * TSTREAM_COLS + lane;
    const bool live = c < C;
    const int entries = H * A;
    unsigned char* mine = state + (long)blockIdx.x * tstream_wave_bytes(entries);
    int* g_head = (int*)mine;
    int* g_cnt = g_head + entries;
    double* g_sum = (double*)(mine + tstream_record_bytes(entries));             // [entry][64]
    float* g_peak = (float*)(g_sum + (long)entries * TSTREAM_COLS);
    float* g_act = g_peak + (long)entries * TSTREAM_COLS;
    for (int i = lane; i < entries; i += 64) {
        s_head[i] = g_head[i];
        s_cnt[i] = g_cnt[i];
    }
    __syncthreads();
    const int lo = slot_base - window > 0 ? slot_base - window : 0;              // the first slot whose smoothed rows this call emits

    // the smoothed rows of slot t, the newest slot in the ring being `newest`: t - window .. min(t + window, newest) are all in the ring
    auto emit = [&](int t, int newest) {
        const int first = t - window > 0 ? t - window : 0;
        const int last = window >= newest - t ? newest : t + window;
        for (int a = 0; a < A; ++a) {
            const int h = s_head[(t % H) * A + a];
            double sum = 0.0;
            int n = 1;
            if (h >= 0) {
                n = 0;
                for (int u = first; u <= last; ++u) {
                    const int e = u % H;
                    const int j = tube_member(s_head + e * A, A, h, lane);
                    if (j < 0) continue;
                    ++n;
                    if (live) sum += (double)g_act[(long)(e * A + j) * TSTREAM_COLS + lane];
                }
            }
            if (live) smooth[((long)(t - lo) * A + a) * C + c] = h >= 0 ? sum / (double)n : 0.0;      // n >= 1: the row itself
        }
    };

    for (int sl = 0; sl < S; ++sl) {
        const int s = slot_base + sl, e = s % H;
        __syncthreads();                                                          // the lookups of the slot before are done with entry e
        if (lane < A) {
            int h = row_head[sl * A + lane];
            if (h < 0 || h > s * A + lane) h = -1;                                // a head is its track's first row
            s_head[e * A + lane] = h;
            s_cnt[e * A + lane] = 0;
        }
        __syncthreads();
        for (int a = 0; a < A; ++a) {
            const int h = s_head[e * A + a];
            const long r = (long)sl * A + a;
            const long at = (long)(e * A + a) * TSTREAM_COLS + lane;
            if (h < 0) {
                if (live) {
                    row_mean[r * C + c] = 0.0;
                    row_peak[r * C + c] = 0.f;
                }
                continue;
            }
            int pe = -1, pa = -1;                                                 // the predecessor: the same head at most max_gap + 1 slots back
            for (int t = s - 1; t >= 0 && t >= s - max_gap - 1; --t) {
                pa = tube_member(s_head + (t % H) * A, A, h, lane);
                if (pa >= 0) { pe = t % H; break; }
            }
            int len = 1;
            if (pe >= 0) len = s_cnt[pe * A + pa] + 1;
            if (lane == a) s_cnt[e * A + a] = len;                                // read at later slots only: a barrier lies in between
            if (live) {
                const float v = actions[r * C + c];
                double tot = 0.0;
                float peak = 0.f;
                if (pe >= 0) {
                    const long from = (long)(pe * A + pa) * TSTREAM_COLS + lane;
                    tot = g_sum[from];
                    peak = g_peak[from];
                }
                tot += (double)v;
                if (len == 1) peak = v;
                else if (peak == peak && (v != v || v > peak)) peak = v;          // np.max: a NaN stays
                g_sum[at] = tot;
                g_peak[at] = peak;
                g_act[at] = v;
                row_mean[r * C + c] = tot / (double)len;
                row_peak[r * C + c] = peak;
            }
        }
        __syncthreads();
        if (lane < A) {
            g_head[e * A + lane] = s_head[e * A + lane];
            g_cnt[e * A + lane] = s_cnt[e * A + lane];
        }
        if (s - window >= 0) emit(s - window, s);                                 // slot s - window has its whole window now
    }
    if (flush) {                                                                  // the end of the video: the last slots take what is there
        const int end = slot_base + S;
        for (int t = end - window > lo ? end - window : lo; t < end; ++t) emit(t, end - 1);
    }
}

// `rows` rows per slot with max_gap: every tube that can be active at one slot finds a lane
static bool tube_active_fit(long rows, long max_gap) { return rows * (max_gap + 1) <= TUBE_MAX_ACTIVE; }

// the size and bound arguments of tuber_tube_link and tuber_tube_link_ranked: TUBER_EINVAL, TUBER_OK for nothing to link, 1 to go on (with the pointers)
static int tube_link_sizes(int V, int S, int N, int C, int max_rows, double link_iou, int max_gap) {
    if (V < 0 || S < 0 || N < 0 || C <= 0 || max_rows < 0 || max_gap < 0 || !(link_iou == link_iou)) return TUBER_EINVAL;
    if (max_rows > FMAP_MAX_DETS || !tube_active_fit(max_rows, max_gap)) return TUBER_EINVAL;
    if ((long)N > (long)S * max_rows || S < V) return TUBER_EINVAL;
    if (N == 0) return TUBER_OK;
    return (long)V * C > 0x7FFFFFFFl ? TUBER_EINVAL : 1;
}

extern "C" {

// tuber_track_actions for ONE video whose key frames arrive in pieces (evaluation.ActorTracker: the definition; video.VideoStream(actors=A)).
// This call takes the S new slots slot_base .. slot_base + S - 1 of A rows each: actions [S * A][C] fp32 and row_head [S * A] as
// tuber_tube_link_stream wrote it for the same slots with C = 1, K = A and the same slot_base.  Out: row_mean [S * A][C] fp64 / row_peak
// [S * A][C] fp32, the track's running mean and maximum after taking the row, and smooth [(hi - lo) * A][C] fp64, the smoothed rows of the slots
// lo = max(slot_base - window, 0) .. hi = flush ? slot_base + S : max(slot_base + S - window, lo) (evaluation.smooth_range); zeros at rows with
// head -1.  state: caller-owned, tuber_track_stream_state_bytes(A, C, max_gap, window) bytes, 16-byte aligned, all zero = a new video; every
// slot writes its ring entry and the kernel knows slot_base, so an entry of an ordinal below 0 or not yet pushed is never consulted.  Refused
// (TUBER_EINVAL, nothing launched, the state untouched, nothing written): A, C or window beyond tuber_track_stream_limits, A * (max_gap + 1)
// beyond tuber_tube_link_max_active(), (slot_base + S) * A beyond an int32, bad sizes, a null or misaligned pointer, negative arguments.
// S == 0 without flush: TUBER_OK, no launch; with flush: the last min(window, slot_base) slots.
int tuber_track_actions_stream(const float* actions, const int* row_head, int S, int A, int C, int slot_base, int max_gap, int window, int flush,
                               void* state, double* row_mean, float* row_peak, double* smooth, hipStream_t stream) {
    if (S < 0 || A < 1 || C < 1 || slot_base < 0 || max_gap < 0 || window < 0 || flush < 0) return TUBER_EINVAL;
    if (A > TUBE_MAX_ACTIVE || C > TRACK_MAX_C || window > TSTREAM_MAX_WINDOW) return TUBER_EINVAL;
    if (!tube_active_fit(A, max_gap) || ((long)slot_base + S) * A > 0x7FFFFFFFl) return TUBER_EINVAL;
    const int H = tstream_slots(max_gap, window);
    if ((long)H * A > TSTREAM_MAX_ENTRIES) return TUBER_EINVAL;                   // cannot happen within the bounds above
    if (!state || ((uintptr_t)state & 15)) return TUBER_EINVAL;
    const long lo = slot_base - window > 0 ? slot_base - window : 0;
    const long end = (long)slot_base + S;
    const long hi = flush ? end : (end - window > lo ? end - window : lo);
    if (S > 0 && (!actions || !row_head || !row_mean || !row_peak)) return TUBER_EINVAL;
    if (hi > lo && !smooth) return TUBER_EINVAL;
    if (S == 0 && hi == lo) return TUBER_OK;                                      // nothing to take and nothing to emit
    hipLaunchKernelGGL(track_actions_stream_kernel, dim3((unsigned)((C + TSTREAM_COLS - 1) / TSTREAM_COLS)), dim3(64), 0, stream, actions, row_head, S,
                       A, C, slot_base, max_gap, window, flush ? 1 : 0, H, (unsigned char*)state, row_mean, row_peak, smooth);
    TUBER_RETURN_LAUNCH();
}
// bytes of the state of tuber_track_actions_stream: per 64 classes H * A head and count records and H * A * 64 (fp64 sum, fp32 peak, fp32
// action) columns, H = max(2 * window, max_gap + 1) + 1; 0 for arguments outside the bounds
long tuber_track_stream_state_bytes(int A, int C, int max_gap, int window) {
    if (A < 1 || C < 1 || max_gap < 0 || window < 0 || A > TUBE_MAX_ACTIVE || C > TRACK_MAX_C || window > TSTREAM_MAX_WINDOW) return 0;
    if (!tube_active_fit(A, max_gap)) return 0;
    const long entries = (long)tstream_slots(max_gap, window) * A;
    if (entries > TSTREAM_MAX_ENTRIES) return 0;
    return (long)((C + TSTREAM_COLS - 1) / TSTREAM_COLS) * tstream_wave_bytes((int)entries);
}
// the bounds of tuber_track_actions_stream: which = 0 the largest A, 1 the largest C, 2 the largest window; anything else -1
int tuber_track_stream_limits(int which) {
    return which == 0 ? TUBE_MAX_ACTIVE : which == 1 ? TRACK_MAX_C : which == 2 ? TSTREAM_MAX_WINDOW : -1;
}

// Per-track and temporally smoothed action scores of linked actor rows (evaluation.actor_tracks: the definition).  actions [S * A][C] fp32, row
// r = slot * A + a; row_head [S * A] / tube_last [S * A] as tuber_tube_link_ranked wrote them for this ONE video with class_num = 1.  Out:
// row_smooth [S * A][C] fp64, the mean over the rows of the row's track at most `window` slots away (fp64 sum in slot order / their number);
// at head rows track_mean [S * A][C] fp64 (fp64 sum in slot order / length) and track_peak [S * A][C] fp32 (maximum); zeros at rows with head
// -1 and, for track_mean / track_peak, at rows that are no head.  A > tuber_track_actions_limits(0), C > tuber_track_actions_limits(1), S * A
// beyond an int32, bad sizes or pointers: TUBER_EINVAL, nothing launched, nothing written.
int tuber_track_actions(const float* actions, const int* row_head, const int* tube_last, int S, int A, int C, int window, double* row_smooth,
                        double* track_mean, float* track_peak, hipStream_t stream) {
    if (S < 0 || A < 1 || C < 1 || window < 0) return TUBER_EINVAL;
    if (A > TUBE_MAX_ACTIVE || C > TRACK_MAX_C || (long)S * A > 0x7FFFFFFFl) return TUBER_EINVAL;
    if (S == 0) return TUBER_OK;
    if (!actions || !row_head || !tube_last || !row_smooth || !track_mean || !track_peak) return TUBER_EINVAL;
    hipLaunchKernelGGL(track_actions_kernel, dim3((unsigned)(S * A)), dim3(TRACK_THREADS), 0, stream, actions, row_head, tube_last, S, A, C, window,
                       row_smooth, track_mean, track_peak);
    TUBER_RETURN_LAUNCH();
}
// the bounds of tuber_track_actions: which = 0 the largest A, 1 the largest C; anything else -1
int tuber_track_actions_limits(int which) { return which == 0 ? TUBE_MAX_ACTIVE : which == 1 ? TRACK_MAX_C : -1; }

// Linking of per-frame detections into action tubes (evaluation.VideoMAP.link).  det_box [N][4] fp32 xyxy / det_prob [N][C + 1] fp32 in layout order
// (video, slot, store order); slot_off DEVICE int[S + 1]: rows per slot; video_off DEVICE int[V + 1]: slots per video.  max_rows: the largest
// number of rows in one slot, which the caller knows.  Refused (negative, nothing launched): max_rows beyond tuber_frame_match_max_dets(),
// max_rows * (max_gap + 1) beyond tuber_tube_link_max_active(), sizes no slot list can meet, bad sizes or pointers.
int tuber_tube_link(const float* det_box, const float* det_prob, const int* slot_off, const int* video_off, int V, int S, int N, int C, int max_rows,
                    double link_iou, int max_gap, int* row_cls, int* row_head, double* tube_score, int* tube_len, int* tube_last,
                    hipStream_t stream) {
    const int rc = tube_link_sizes(V, S, N, C, max_rows, link_iou, max_gap);
    if (rc != 1) return rc;
    if (!det_box || !det_prob || !slot_off || !video_off || !row_cls || !row_head || !tube_score || !tube_len || !tube_last) return TUBER_EINVAL;
    hipLaunchKernelGGL(tube_rows_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, det_prob, N, C, row_cls, row_head);
    const long waves = (long)V * C;
    hipLaunchKernelGGL((tube_link_kernel<false, false>), dim3((unsigned)((waves + TLINK_WAVES - 1) / TLINK_WAVES)), dim3(64 * TLINK_WAVES), 0, stream, det_box,
                       det_prob, slot_off, video_off, V, S, N, C, link_iou, max_gap, row_cls, row_head, tube_score, tube_len, tube_last, 0, 0,
                       (unsigned char*)nullptr);
    TUBER_RETURN_LAUNCH();
}

// tuber_tube_link over ranked detections (detect.Detections, video.VideoDetections): a row's class and score are det_label [N] (0-based; negative or
// >= C: the row is not counted) and det_score [N] fp32 instead of the arg-max of a [N][C + 1] row.  Everything else -- arguments, outputs, bounds,
// negative codes, the walk and the fp64 sequential mean -- is tuber_tube_link's; row_cls: the label, C for a row that is not counted.
int tuber_tube_link_ranked(const float* det_box, const int* det_label, const float* det_score, const int* slot_off, const int* video_off, int V, int S,
                           int N, int C, int max_rows, double link_iou, int max_gap, int* row_cls, int* row_head, double* tube_score, int* tube_len,
                           int* tube_last, hipStream_t stream) {
    const int rc = tube_link_sizes(V, S, N, C, max_rows, link_iou, max_gap);
    if (rc != 1) return rc;
    if (!det_box || !det_label || !det_score || !slot_off || !video_off || !row_cls || !row_head || !tube_score || !tube_len || !tube_last)
        return TUBER_EINVAL;
    hipLaunchKernelGGL(tube_rows_ranked_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, det_label, N, C, row_cls, row_head);
    const long waves = (long)V * C;
    hipLaunchKernelGGL((tube_link_kernel<true, false>), dim3((unsigned)((waves + TLINK_WAVES - 1) / TLINK_WAVES)), dim3(64 * TLINK_WAVES), 0, stream, det_box,
                       det_score, slot_off, video_off, V, S, N, C, link_iou, max_gap, row_cls, row_head, tube_score, tube_len, tube_last, 0, 0,
                       (unsigned char*)nullptr);
    TUBER_RETURN_LAUNCH();
}
int tuber_tube_link_max_active() { return TUBE_MAX_ACTIVE; }

// tuber_tube_link_ranked for ONE video whose slots arrive in pieces (evaluation.TubeLinker: the definition; video.VideoStream).  This call links
// the S new slots with the ordinals slot_base .. slot_base + S - 1, K rows each (det_box [S * K][4], det_label / det_score [S * K]; the rows
// behind a key's count carry label -1).  state: caller-owned, tuber_tube_link_state_bytes(C) bytes, 16-byte aligned, all zero = no tubes; loaded
// before the walk and stored after it.  Out, per row: row_head the GLOBAL row (ordinal * K + position) of the tube's first detection, row_score
// the tube's fp64 mean and row_len its count after taking the row; -1, 0, 0 for a row that is not counted.  Refused (TUBER_EINVAL, nothing
// launched, the state untouched): K > tuber_frame_match_max_dets(), K * (max_gap + 1) > tuber_tube_link_max_active(), (slot_base + S) * K beyond
// an int32, bad sizes or pointers.
int tuber_tube_link_stream(const float* det_box, const int* det_label, const float* det_score, int S, int K, int slot_base, int C, double link_iou,
                           int max_gap, void* state, int* row_head, double* row_score, int* row_len, hipStream_t stream) {
    if (S < 0 || K <= 0 || slot_base < 0 || C <= 0 || max_gap < 0 || !(link_iou == link_iou)) return TUBER_EINVAL;
    if (K > FMAP_MAX_DETS || !tube_active_fit(K, max_gap)) return TUBER_EINVAL;
    if (((long)slot_base + S) * K > 0x7FFFFFFFl || (long)C * 64 * TUBE_STATE_LANE_BYTES > 0x7FFFFFFFl) return TUBER_EINVAL;
    if (!state || ((uintptr_t)state & 15)) return TUBER_EINVAL;
    if (S == 0) return TUBER_OK;
    if (!det_box || !det_label || !det_score || !row_head || !row_score || !row_len) return TUBER_EINVAL;
    const int N = S * K;
    hipLaunchKernelGGL(tube_rows_stream_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, N, row_head, row_score, row_len);
    hipLaunchKernelGGL((tube_link_kernel<true, true>), dim3((unsigned)((C + TLINK_WAVES - 1) / TLINK_WAVES)), dim3(64 * TLINK_WAVES), 0, stream, det_box,
                       det_score, (const int*)nullptr, (const int*)nullptr, 1, S, N, C, link_iou, max_gap, det_label, row_head, row_score, row_len,
                       (int*)nullptr, K, slot_base, (unsigned char*)state);
    TUBER_RETURN_LAUNCH();
}
long tuber_tube_link_state_bytes(int C) { return C > 0 ? (long)C * 64 * TUBE_STATE_LANE_BYTES : 0; }

// Spatio-temporal matching of the linked tubes against the ground-truth tubes (evaluation.VideoMAP.match).  The link outputs; gt_box [G][4] fp64,
// gt_cls [G], gt_tube [G] (the rank of the row's tube among the tube ids of its (video, class), ascending; one row per (slot, class, tube)) in slot
// order, gt_off DEVICE int[S + 1]; thresholds DEVICE double[T]; work: caller-owned double[N * max(max_gt_tubes, 1)].  max_rows, max_gt_rows,
// max_gt_tubes: the largest rows / ground-truth rows per slot and ground-truth tubes per (video, class), which the caller knows.  tube_flag [T][N]
// bytes out: 1 true positive, 0 false positive, 2 not counted (not a head, or shorter than min_len), 3 a (video, class) beyond the bounds.
int tuber_tube_match(const float* det_box, const int* slot_off, const int* video_off, const int* row_cls, const int* row_head,
                     const double* tube_score, const int* tube_len, const int* tube_last, const double* gt_box, const int* gt_cls,
                     const int* gt_tube, const int* gt_off, const double* thresholds, int V, int S, int N, int G, int C, int T, int max_rows,
                     int max_gt_rows, int max_gt_tubes, int min_len, double* work, unsigned char* tube_flag, hipStream_t stream) {
    if (V < 0 || S < 0 || N < 0 || G < 0 || C <= 0 || T <= 0 || max_rows < 0 || max_gt_rows < 0 || max_gt_tubes < 0) return TUBER_EINVAL;
    if (T > TUBE_MAX_THR || max_gt_tubes > TUBE_MAX_GT || max_rows > FMAP_MAX_DETS || max_gt_rows > FMAP_MAX_GT) return TUBER_EINVAL;
    if ((long)N > (long)S * max_rows || (long)G > (long)S * max_gt_rows || S < V) return TUBER_EINVAL;
    if (N == 0) return TUBER_OK;
    if ((long)V * C > 0x7FFFFFFFl || (long)T * N > 0x7FFFFFFFl) return TUBER_EINVAL;
    if (!det_box || !slot_off || !video_off || !row_cls || !row_head || !tube_score || !tube_len || !tube_last || !gt_off || !thresholds || !work ||
        !tube_flag)
        return TUBER_EINVAL;
    if (G > 0 && (!gt_box || !gt_cls || !gt_tube)) return TUBER_EINVAL;
    const hipError_t e = hipMemsetAsync(tube_flag, TUBE_NOT_COUNTED, (size_t)T * N, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(tube_match_kernel, dim3((unsigned)(V * C)), dim3(64), 0, stream, det_box, slot_off, video_off, row_cls, row_head, tube_score,
                       tube_len, tube_last, gt_box, gt_cls, gt_tube, gt_off, thresholds, S, N, G, C, T, max_gt_tubes, min_len, work, tube_flag);
    TUBER_RETURN_LAUNCH();
}
// Spatio-temporal NMS over linked tubes (evaluation.tube_nms: the definition).  The operands are the link outputs as tuber_tube_match reads them:
// the validation store in layout order, or a padded [S][K] store with slot_off = arange(S + 1) * K and V = 1.  Two tubes of one (video, class)
// overlap by stIoU = sum over the shared slots, ascending, of the fp64 IoU / |slots of either|; the tubes of at least min_len detections are
// visited by descending score (NaN last, equal scores by ascending head) and one is suppressed iff its stIoU with a tube kept before it is
// > nms_iou.  tube_keep [N] bytes out: 1 kept head, 0 suppressed head, 2 not a head or shorter than min_len, 3 at the heads of a (video, class)
// with more than tuber_tube_link_max_active() tubes live at one slot.  work: caller-owned, tuber_tube_nms_work_bytes(N) bytes, 16-byte aligned.
// Refused (negative, nothing launched, nothing written): max_rows > tuber_frame_match_max_dets(), min_len < 1, nms_iou NaN or outside [0, 1],
// N > S * max_rows, bad sizes, a null pointer or a misaligned work.
int tuber_tube_nms(const float* det_box, const int* slot_off, const int* video_off, const int* row_cls, const int* row_head,
                   const double* tube_score, const int* tube_len, const int* tube_last, int V, int S, int N, int C, int max_rows, int min_len,
                   double nms_iou, void* work, unsigned char* tube_keep, hipStream_t stream) {
    if (V < 0 || S < 0 || N < 0 || C <= 0 || max_rows < 0 || min_len < 1) return TUBER_EINVAL;
    if (!(nms_iou >= 0.0 && nms_iou <= 1.0)) return TUBER_EINVAL;                // a NaN fails both comparisons
    if (max_rows > FMAP_MAX_DETS || (long)N > (long)S * max_rows || S < V) return TUBER_EINVAL;
    if ((long)V * C > 0x7FFFFFFFl) return TUBER_EINVAL;
    if (N == 0 || V == 0) return TUBER_OK;
    if (!det_box || !slot_off || !video_off || !row_cls || !row_head || !tube_score || !tube_len || !tube_last || !work || !tube_keep)
        return TUBER_EINVAL;
    if ((uintptr_t)work & 15) return TUBER_EINVAL;
    const hipError_t e = hipMemsetAsync(tube_keep, TUBE_NOT_COUNTED, (size_t)N, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(tube_nms_kernel, dim3((unsigned)(V * C)), dim3(64), 0, stream, det_box, slot_off, video_off, row_cls, row_head, tube_score,
                       tube_len, tube_last, S, N, C, min_len, nms_iou, (int*)work, tube_keep);
    TUBER_RETURN_LAUNCH();
}
// bytes of the scratch of tuber_tube_nms: per row 64 partner heads and one status word (int32), rounded up to 16 bytes; 0 for N <= 0
long tuber_tube_nms_work_bytes(long N) { return N > 0 ? (N * (TNMS_ROW + 1) * 4 + 15) & ~15l : 0; }

// Dense tubes (evaluation.dense_rows: the definition): per-frame boxes and scores between the linked key detections of ONE video's padded
// [S][K] store.  det_box [S * K][4] / det_score [S * K] fp32, row_head [S * K] as tuber_tube_link_ranked wrote it, slot_frame [S] the frame
// number of every key ordinal (strictly ascending), G >= the most frames a row can own (evaluation.dense_extent: a host integer).  Out, per
// row r: row_next the first row with r's head in the next max_gap + 1 slots (-1: none), row_span g = the frames between the two keys (1
// without a successor, 0 for a row with head < 0, whose row_next is -1), dense_box [S * K][G][4] / dense_score [S * K][G] at j < g: the
// row's own bytes at j = 0, float(double(a) + (double(b) - double(a)) * (double(j) / double(g))) behind it; nothing is written at j >= g.
// g < 1 or g > G (unsorted slot_frame, a G too small): row_span -1 and nothing else -- the caller answers with the definition.  Refused
// (TUBER_EINVAL, nothing launched, nothing written): K > tuber_frame_match_max_dets(), K * (max_gap + 1) > tuber_tube_link_max_active(),
// S * K * G beyond an int32, G < 1, K < 1, negative sizes, a null pointer, det_box / dense_box not 16-byte or another pointer not 4-byte
// aligned.  S == 0: TUBER_OK, no launch.
int tuber_tube_dense(const float* det_box, const float* det_score, const int* row_head, const int* slot_frame, int S, int K, int max_gap, int G,
                     float* dense_box, float* dense_score, int* row_span, int* row_next, hipStream_t stream) {
    if (S < 0 || K < 1 || max_gap < 0 || G < 1) return TUBER_EINVAL;
    if (K > FMAP_MAX_DETS || !tube_active_fit(K, max_gap)) return TUBER_EINVAL;
    if ((long)S * K > 0x7FFFFFFFl || (long)S * K * G > 0x7FFFFFFFl) return TUBER_EINVAL;
    if (S == 0) return TUBER_OK;
    if (!det_box || !det_score || !row_head || !slot_frame || !dense_box || !dense_score || !row_span || !row_next) return TUBER_EINVAL;
    if (((uintptr_t)det_box & 15) || ((uintptr_t)dense_box & 15)) return TUBER_EINVAL;
    if (((uintptr_t)det_score | (uintptr_t)row_head | (uintptr_t)slot_frame | (uintptr_t)dense_score | (uintptr_t)row_span | (uintptr_t)row_next) & 3)
        return TUBER_EINVAL;
    const long N = (long)S * K;
    hipLaunchKernelGGL(tube_dense_kernel, dim3((unsigned)((N + TDENSE_WAVES - 1) / TDENSE_WAVES)), dim3(64 * TDENSE_WAVES), 0, stream, det_box, det_score,
                       row_head, slot_frame, S, K, max_gap, G, dense_box, dense_score, row_span, row_next);
    TUBER_RETURN_LAUNCH();
}

int tuber_tube_match_max_gt() { return TUBE_MAX_GT; }
int tuber_tube_match_max_thresholds() { return TUBE_MAX_THR; }

}  // extern "C"
