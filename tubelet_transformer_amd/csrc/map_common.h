// Helpers the evaluation kernels share (frame_map.hip, tube_map.hip): the fp64 IoU that decides "IoU >= threshold" exactly as the host evaluators
// do, the order key of (score, row), and the np.argmax of a probability row.  Both sources are built with -ffp-contract=on (build.py), under which
// the pragma below holds.
#pragma once
#include "common.h"

#define FMAP_MAX_DETS 64          // detections per frame: the valid set is one 64-bit mask, a row index fits the low word of the order key
#define FMAP_MAX_GT 32            // ground-truth boxes per frame: candidate and taken sets are 32-bit masks

// IoU of two boxes in fp64, expression for expression evaluation._iou_one_to_many; no FMA contraction, so that a decision at exactly the
// threshold falls as it does on the host
__device__ __forceinline__ double fmap_iou_d(double b0, double b1, double b2, double b3, double g0, double g1, double g2, double g3) {
#pragma clang fp contract(off)
    const double x1 = fmax(b0, g0), y1 = fmax(b1, g1), x2 = fmin(b2, g2), y2 = fmin(b3, g3);
    const double w = fmax(x2 - x1, 0.0), h = fmax(y2 - y1, 0.0);
    const double inter = w * h;
    const double a = (b2 - b0) * (b3 - b1);
    const double b = (g2 - g0) * (g3 - g1);
    const double u = a + b;
    return inter / (u - inter);
}

// an fp32 detection box with an fp64 ground-truth box
__device__ __forceinline__ double fmap_iou(const float* __restrict__ d, const double* __restrict__ g) {
    return fmap_iou_d((double)d[0], (double)d[1], (double)d[2], (double)d[3], g[0], g[1], g[2], g[3]);
}

// order key of (score, row in frame): a larger key is visited earlier.  High word: the score as an order-preserving unsigned (-0 == +0, NaN below
// everything: np.argsort(-score) puts NaN last); low word: ~row, so equal scores go by ascending row.
__device__ __forceinline__ unsigned long long fmap_key(float s, int k) {
    unsigned u = __float_as_uint(s);
    if (s != s) u = 0u;
    else {
        if (s == 0.f) u = 0u;
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)k);
}

// np.argmax over the C + 1 columns of a probability row (the first maximum, a NaN counting as one); score: that column's value
__device__ __forceinline__ int fmap_argmax(const float* __restrict__ p, int C, float& score) {
    int a = 0;
    score = p[0];
    for (int c = 1; c <= C; ++c) {
        const float v = p[c];
        if (score == score && (v > score || v != v)) { a = c; score = v; }
    }
    return a;
}
