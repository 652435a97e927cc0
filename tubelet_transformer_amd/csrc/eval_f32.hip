// fp32 kernels of the EVAL precision mode (round 6): the DETR decoder stack and the box / actor heads in fp32.
// reference: TransformerDecoder / TransformerDecoderLayer.forward_post (models/transformer/transformer.py:99-128,218-249), the heads of
// DETR.forward (models/tuber_ava.py:121-125,142), MLP (models/criterion.py:485-497).
//
// Why: eval has no batch statistics and is not the throughput metric, and the published numbers of the reference (mAP 29.7 / 31.1) live
// there.  The bf16 path's error on the actor logits is carried in roughly equal parts by the body's convs, the decoder's linears and the
// heads (measured on the oracle with selective rounding); the decoder works on <= 640 rows x 256 -- a few MFLOP per
// layer -- so it runs in fp32 outright under model.eval(): fp32 MFMA / FMA kernels, fp32 master weights straight from the flat parameter
// buffer, fp32 softmax, the residual stream never rounded.  The 704-row memory-side projections are the only part with real work
// (185 MFLOP per layer).  Training keeps the bf16 MFMA path (tuber_decoder_coop_fwd / the launch chain).
//
// TUBER_EVAL_PRECISION=fp32_class (round 7) also runs the class branch (tuber_ava.py:127-141, transformer_layers.py:71-97) here, ONCE per
// clip instead of once per decoder layer: its attention cores read their operands through the token maps of tuber_attn_fwd
// (tuber_attention_f32_mapped), its LayerNorms write into the halves of the [t | s] feature concatenation (tuber_layernorm_f32_rows).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

// y[m][n] = act( sum_k (x[m][k] + (n < add_cols ? add[m][k] : 0)) * W[n][k] + bias[n] ),  act: 0 none, 1 ReLU, 2 sigmoid -- on the fp32
// matrix pipe (v_mfma_f32_16x16x4_f32 / v_mfma_f32_32x32x2_f32: true fp32 multiply-adds), operand fragments straight from global memory:
// a lane holds 4 consecutive k of one row (one 16-byte load) and feeds them to 4 MFMAs -- which k a lane group contributes to which MFMA
// does not matter as long as both operands agree.  blockIdx.z walks a batch of weight sets (the six layers' memory projections).
struct LinArgs {
    const float* x; long ldx; const float* add; long ldadd; int add_cols;
    const float* W; long ldw; const float* bias; float* y; long ldy;
    int M, N, K, act; long wz, bz, yz;
};

__device__ __forceinline__ float lin_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return 1.f / (1.f + expf(-v));
    return v;
}

constexpr int LIN_PF = 8;          // k steps of operand loads in flight per wave

// FEW ROWS (the decoder's 30, the heads' 180): a workgroup owns ONE 16 x 16 output tile and its four waves take every fourth 16-wide k
// chunk -- the first version (32 x 64 LDS tiles, FMA from broadcast reads) ran the decoder's 30-row layers as one latency chain of K / 32
// fetch -> park -> FMA rounds on 4 workgroups (~16 us per layer call); here a 30 x 256 x 256 layer is 32 workgroups of 4 + 4 loads per lane.
// The four partial tiles meet in LDS and are summed in wave order (deterministic).
__global__ __launch_bounds__(256) void linear_f32_rows_kernel(LinArgs a) {
    __shared__ float red[4][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 16;
    const int r = lane & 15, kq = lane >> 4;
    const bool with_add = a.add != nullptr && n0 < a.add_cols;
    const float* xp = a.x + (long)min(m0 + r, a.M - 1) * a.ldx + 4 * kq;
    const float* ap = with_add ? a.add + (long)min(m0 + r, a.M - 1) * a.ldadd + 4 * kq : nullptr;
    const float* wp = a.W + blockIdx.z * a.wz + (long)min(n0 + r, a.N - 1) * a.ldw + 4 * kq;
    const int nchunks = a.K >> 4;
    const int ns = nchunks > w ? (nchunks - w + 3) >> 2 : 0;          // chunks w, w + 4, ...
    float4 xa[LIN_PF], wb[LIN_PF];
    auto ld = [&](int s, float4& xv, float4& wv) {
        const long k0 = 16L * min(4 * s + w, nchunks - 1);
        xv = *(const float4*)(xp + k0);
        if (with_add) { const float4 t = *(const float4*)(ap + k0); xv.x += t.x; xv.y += t.y; xv.z += t.z; xv.w += t.w; }
        wv = *(const float4*)(wp + k0);
    };
#pragma unroll
    for (int u = 0; u < LIN_PF; ++u) ld(u, xa[u], wb[u]);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < ns; s0 += LIN_PF) {
#pragma unroll
        for (int u = 0; u < LIN_PF; ++u) {
            if (s0 + u < ns) {
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u].x, wb[u].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u].y, wb[u].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u].z, wb[u].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u].w, wb[u].w, acc, 0, 0, 0);
            }
            if (s0 + u + LIN_PF < ns) ld(s0 + u + LIN_PF, xa[u], wb[u]);
        }
    }
    // D[i][j]: j = lane % 16, i = 4 * (lane / 16) + v
#pragma unroll
    for (int v = 0; v < 4; ++v) red[w][(4 * kq + v) * 16 + r] = acc[v];
    __syncthreads();
    const int m = m0 + (tid >> 4), n = n0 + (tid & 15);
    if (m < a.M && n < a.N) {
        float v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        if (a.bias) v += a.bias[blockIdx.z * a.bz + n];
        a.y[blockIdx.z * a.yz + (long)m * a.ldy + n] = lin_act(v, a.act);
    }
}

// MANY ROWS (the 704-row memory projections): 64 x 64 per workgroup, a wave owns a 32 x 32 block over the whole reduction.
__global__ __launch_bounds__(256) void linear_f32_tile_kernel(LinArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = blockIdx.x * 64 + (w >> 1) * 32, n0 = blockIdx.y * 64 + (w & 1) * 32;
    if (m0 >= a.M || n0 >= a.N) return;
    const int r = lane & 31, kh = lane >> 5;
    const bool with_add = a.add != nullptr && n0 < a.add_cols;
    const float* xp = a.x + (long)min(m0 + r, a.M - 1) * a.ldx + 4 * kh;
    const float* ap = with_add ? a.add + (long)min(m0 + r, a.M - 1) * a.ldadd + 4 * kh : nullptr;
    const float* wp = a.W + blockIdx.z * a.wz + (long)min(n0 + r, a.N - 1) * a.ldw + 4 * kh;
    const int ns = a.K >> 3;
    float4 xa[LIN_PF], wb[LIN_PF];
    auto ld = [&](int s, float4& xv, float4& wv) {
        const long k0 = 8L * min(s, ns - 1);
        xv = *(const float4*)(xp + k0);
        if (with_add) { const float4 t = *(const float4*)(ap + k0); xv.x += t.x; xv.y += t.y; xv.z += t.z; xv.w += t.w; }
        wv = *(const float4*)(wp + k0);
    };
#pragma unroll
    for (int u = 0; u < LIN_PF; ++u) ld(u, xa[u], wb[u]);
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    for (int s0 = 0; s0 < ns; s0 += LIN_PF) {
#pragma unroll
        for (int u = 0; u < LIN_PF; ++u) {
            if (s0 + u < ns) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u].x, wb[u].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u].y, wb[u].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u].z, wb[u].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u].w, wb[u].w, acc, 0, 0, 0);
            }
            if (s0 + u + LIN_PF < ns) ld(s0 + u + LIN_PF, xa[u], wb[u]);
        }
    }
    // D[i][j]: j = lane % 32, i = 8 * (v / 4) + 4 * (lane / 32) + v % 4
    const int n = n0 + r;
    if (n >= a.N) return;
    const float b = a.bias ? a.bias[blockIdx.z * a.bz + n] : 0.f;
    float* yp = a.y + blockIdx.z * a.yz + n;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int m = m0 + 8 * (v >> 2) + 4 * kh + (v & 3);
        if (m < a.M) yp[(long)m * a.ldy] = lin_act(acc[v] + b, a.act);
    }
}

// token map of an attention operand (tuber_attn_fwd's {ld, sL, s1, s2, B2}): token l of sequence b sits in row l * sL + (b / B2) * s1 + (b % B2) * s2
// of a row-major matrix with leading dimension ld (elements).  The dense (b, l) layout is {ld, 1, L, 0, 1}.
struct RowMap { long ld, sL, s1, s2; int B2; };

__device__ __forceinline__ long map_row0(const RowMap& m, int b) { return ((long)(b / m.B2) * m.s1 + (long)(b % m.B2) * m.s2) * m.ld; }

// one workgroup per (sequence b, head h, chunk of <= QCAP queries): o(i, b)[h*D + d] = sum_j softmax_j(scale * q(i, b) . k(j, b)) v(j, b)[d], keys
// masked by kpm[b][j] != 0; rows through the token maps mq / mk / mv / mo; D = 32.  The queries of the chunk share every K / V row: thread t scores key
// j = t, t + 256, ... against all of them (its K row in registers, the queries as LDS broadcasts) into the LDS score table [QCAP][Lk]; a wave per
// query takes max / exp / sum; then thread (key slice t / 32, d = t % 32) accumulates P . V for ALL queries over every eighth key -- 8 value rows
// in flight per thread, 64 per workgroup, the first batch (like the first K row) fetched before anything else -- and the eight partial sums meet in LDS
// in slice order.  History: one wave per (b, h, query) re-read the same 90 KB of K / V fifteen times and walked the keys as one dependent chain;
// the first shared form kept the V walk per query group (44 exposed round trips: 69 us per cross-attention call at 15 x 352).
template <int QCAP>
__global__ __launch_bounds__(256) void attention_f32_kernel(const float* __restrict__ q, RowMap mq, const float* __restrict__ k, RowMap mk,
                                                            const float* __restrict__ v, RowMap mv, float* __restrict__ o, RowMap mo,
                                                            const uint8_t* __restrict__ kpm, int H, int LqAll, int Lk, float scale) {
    constexpr int D = 32;
    extern __shared__ __attribute__((aligned(16))) float sm[];     // [QCAP][D] queries (pre-scaled), [QCAP] 1 / l, [8][QCAP][D] partial outputs, [QCAP][Lk] scores -> probabilities
    float* qs = sm;
    float* linv = sm + QCAP * D;
    float* red = linv + QCAP;
    float* sc = red + 8 * QCAP * D;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nqc = (LqAll + QCAP - 1) / QCAP;
    int u0 = blockIdx.x;
    const int i0 = (u0 % nqc) * QCAP; u0 /= nqc;
    const int h = u0 % H, b = u0 / H;
    const int Lq = min(QCAP, LqAll - i0);
    const long ldq = mq.sL * mq.ld, ldk = mk.sL * mk.ld, ldv = mv.sL * mv.ld, ldo = mo.sL * mo.ld;      // element strides between tokens
    q += map_row0(mq, b) + i0 * ldq;
    o += map_row0(mo, b) + i0 * ldo;
    const float* kb = k + map_row0(mk, b) + h * D;
    const int d = tid & 31, ks = tid >> 5;
    const float* vp = v + map_row0(mv, b) + h * D + d;
    // everything that does not depend on another thread is requested first: this thread's first K row and first batch of V rows
    float kr[D], vv[8];
    {
        const float* kp = kb + (long)min(tid, Lk - 1) * ldk;
#pragma unroll
        for (int e = 0; e < D; e += 4) { const float4 t = *(const float4*)(kp + e); kr[e] = t.x; kr[e + 1] = t.y; kr[e + 2] = t.z; kr[e + 3] = t.w; }
#pragma unroll
        for (int t = 0; t < 8; ++t) vv[t] = vp[(long)min(ks + 8 * t, Lk - 1) * ldv];
    }
    for (int e = tid; e < QCAP * D; e += 256) qs[e] = e < Lq * D ? q[(long)(e / D) * ldq + h * D + (e % D)] * scale : 0.f;
    __syncthreads();
    for (int j = tid; j < Lk; j += 256) {
        if (j != tid) {
            const float* kp = kb + (long)j * ldk;
#pragma unroll
            for (int e = 0; e < D; e += 4) { const float4 t = *(const float4*)(kp + e); kr[e] = t.x; kr[e + 1] = t.y; kr[e + 2] = t.z; kr[e + 3] = t.w; }
        }
        const bool masked = kpm && kpm[(long)b * Lk + j];
        for (int i = 0; i < Lq; ++i) {
            const float4* q4 = (const float4*)(qs + i * D);
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < D; e += 4) {
                const float4 t = q4[e >> 2];
                s = fmaf(t.x, kr[e], s); s = fmaf(t.y, kr[e + 1], s); s = fmaf(t.z, kr[e + 2], s); s = fmaf(t.w, kr[e + 3], s);
            }
            sc[i * Lk + j] = masked ? -INFINITY : s;
        }
    }
    __syncthreads();
    for (int i = w; i < QCAP; i += 4) {
        float* row = sc + i * Lk;
        if (i >= Lq) {                                 // unused rows of the chunk: zero probabilities, so the P . V walk needs no bounds on i
            for (int j = lane; j < Lk; j += 64) row[j] = 0.f;
            continue;
        }
        float mx = -INFINITY;
        for (int j = lane; j < Lk; j += 64) mx = fmaxf(mx, row[j]);
        mx = wave_max(mx);
        float l = 0.f;
        for (int j = lane; j < Lk; j += 64) { const float p = expf(row[j] - mx); row[j] = p; l += p; }
        l = wave_sum(l);
        if (lane == 0) linv[i] = 1.f / l;
    }
    __syncthreads();
    float acc[QCAP];
#pragma unroll
    for (int i = 0; i < QCAP; ++i) acc[i] = 0.f;
    for (int j0 = ks; j0 < Lk; j0 += 64) {             // keys j0, j0 + 8, ..., j0 + 56 of this slice
        float cur[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) cur[t] = vv[t];
        if (j0 + 64 < Lk) {
#pragma unroll
            for (int t = 0; t < 8; ++t) vv[t] = vp[(long)min(j0 + 64 + 8 * t, Lk - 1) * ldv];
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int j = j0 + 8 * t;
            if (j < Lk) {
#pragma unroll
                for (int i = 0; i < QCAP; ++i) acc[i] = fmaf(sc[i * Lk + j], cur[t], acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < QCAP; ++i) red[(ks * QCAP + i) * D + d] = acc[i];
    __syncthreads();
    for (int e = tid; e < Lq * D; e += 256) {
        float r = 0.f;
#pragma unroll
        for (int sl = 0; sl < 8; ++sl) r += red[sl * QCAP * D + e];
        o[(long)(e / D) * ldo + h * D + (e % D)] = r * linv[e / D];
    }
}

// SHORT sequences (Lq, Lk <= LMAX: the class branch's s-attention over T' = 4 frames): the problem is nothing but (sequence, head) pairs --
// 2 x 352 x 8 for config 3 -- so a thread owns one (b, i, h) query row end to end: its 32-wide q row, <= LMAX scores and softmax in
// registers, the P . V sum over the same <= LMAX rows.  h runs fastest across the lanes, so 8 lanes read one 1 KB operand row.
template <int LMAX>
__global__ __launch_bounds__(256) void attention_f32_short_kernel(const float* __restrict__ q, RowMap mq, const float* __restrict__ k, RowMap mk,
                                                                  const float* __restrict__ v, RowMap mv, float* __restrict__ o, RowMap mo,
                                                                  int B, int H, int Lq, int Lk, float scale) {
    constexpr int D = 32;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * Lq * H) return;
    const int h = (int)(t % H);
    const long u = t / H;
    const int i = (int)(u % Lq), b = (int)(u / Lq);
    const float* qp = q + map_row0(mq, b) + i * mq.sL * mq.ld + h * D;
    const float* kp = k + map_row0(mk, b) + h * D;
    const float* vp = v + map_row0(mv, b) + h * D;
    const long ldk = mk.sL * mk.ld, ldv = mv.sL * mv.ld;
    float qr[D];
#pragma unroll
    for (int e = 0; e < D; e += 4) { const float4 x = *(const float4*)(qp + e); qr[e] = x.x * scale; qr[e + 1] = x.y * scale; qr[e + 2] = x.z * scale; qr[e + 3] = x.w * scale; }
    float s[LMAX], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < LMAX; ++j) {
        s[j] = -INFINITY;
        if (j < Lk) {
            const float* kr = kp + j * ldk;
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < D; e += 4) {
                const float4 x = *(const float4*)(kr + e);
                a = fmaf(qr[e], x.x, a); a = fmaf(qr[e + 1], x.y, a); a = fmaf(qr[e + 2], x.z, a); a = fmaf(qr[e + 3], x.w, a);
            }
            s[j] = a;
            mx = fmaxf(mx, a);
        }
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < LMAX; ++j) { s[j] = j < Lk ? expf(s[j] - mx) : 0.f; l += s[j]; }
    float acc[D];
#pragma unroll
    for (int e = 0; e < D; ++e) acc[e] = 0.f;
#pragma unroll
    for (int j = 0; j < LMAX; ++j) {
        if (j < Lk) {
            const float* vr = vp + j * ldv;
#pragma unroll
            for (int e = 0; e < D; e += 4) {
                const float4 x = *(const float4*)(vr + e);
                acc[e] = fmaf(s[j], x.x, acc[e]); acc[e + 1] = fmaf(s[j], x.y, acc[e + 1]); acc[e + 2] = fmaf(s[j], x.z, acc[e + 2]); acc[e + 3] = fmaf(s[j], x.w, acc[e + 3]);
            }
        }
    }
    const float li = 1.f / l;
    float* op = o + map_row0(mo, b) + i * mo.sL * mo.ld + h * D;
#pragma unroll
    for (int e = 0; e < D; e += 4) *(float4*)(op + e) = make_float4(acc[e] * li, acc[e + 1] * li, acc[e + 2] * li, acc[e + 3] * li);
}

// y = LayerNorm(x + res) over E = 256, all fp32, every operand with its own leading dimension: one wave per row, 4 consecutive columns per lane
__global__ __launch_bounds__(256) void layernorm_f32_rows_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ res, long ldr,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y,
                                                                 long ldy, int M, float eps) {
    constexpr int E = 256;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int col = 4 * lane;
    float4 a = *(const float4*)(x + (long)row * ldx + col);
    if (res) { const float4 r = *(const float4*)(res + (long)row * ldr + col); a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w; }
    const float mean = wave_sum((a.x + a.y) + (a.z + a.w)) * (1.f / E);
    const float d0 = a.x - mean, d1 = a.y - mean, d2 = a.z - mean, d3 = a.w - mean;
    const float rstd = rsqrtf(wave_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * (1.f / E) + eps);
    const float4 g = *(const float4*)(gamma + col), bb = *(const float4*)(beta + col);
    *(float4*)(y + (long)row * ldy + col) = make_float4(fmaf(d0 * rstd, g.x, bb.x), fmaf(d1 * rstd, g.y, bb.y), fmaf(d2 * rstd, g.z, bb.z), fmaf(d3 * rstd, g.w, bb.w));
}

}  // namespace

extern "C" {

static int linear_f32_launch(const float* x, long ldx, const float* add, long ldadd, int add_cols, const float* W, long ldw, const float* bias,
                             float* y, long ldy, int M, int N, int K, int act, int nbatch, long wz, long bz, long yz, hipStream_t stream) {
    if (!x || !W || !y || M <= 0 || N <= 0 || K <= 0 || (K & 31) || (ldx & 3) || (ldw & 3) || (wz & 3) || (add && ((ldadd & 3) || (add_cols & 63))) || act < 0 || act > 2 ||
        nbatch <= 0 || nbatch > 65535)
        return TUBER_EINVAL;
    LinArgs a{x, ldx, add, ldadd, add ? add_cols : 0, W, ldw, bias, y, ldy, M, N, K, act, wz, bz, yz};
    if (M <= 256)
        hipLaunchKernelGGL(linear_f32_rows_kernel, dim3(ceil_div(M, 16), ceil_div(N, 16), nbatch), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(linear_f32_tile_kernel, dim3(ceil_div(M, 64), ceil_div(N, 64), nbatch), dim3(256), 0, stream, a);
    TUBER_RETURN_LAUNCH();
}

// fp32 linear layer y = act((x [+ add for the output columns < add_cols]) . W^T + bias): x [M, K] (ldx), add [M, K] or NULL (with_pos_embed:
// the q / k rows of a packed in-projection see x + pos, the v rows x), W [N, K] (ldw) and bias [N] fp32 -- the master parameters --,
// y [M, N] (ldy).  act: 0 none, 1 ReLU, 2 sigmoid.  K % 32 == 0, add_cols % 64 == 0, 16-byte aligned rows.
int tuber_linear_f32(const float* x, long ldx, const float* add, long ldadd, int add_cols, const float* W, long ldw, const float* bias,
                     float* y, long ldy, int M, int N, int K, int act, hipStream_t stream) {
    return linear_f32_launch(x, ldx, add, ldadd, add_cols, W, ldw, bias, y, ldy, M, N, K, act, 1, 0, 0, 0, stream);
}

// the same layer for `nbatch` weight sets over ONE input in one launch: set z reads W + z * w_stride, bias + z * bias_stride and writes
// y + z * y_stride (strides in elements) -- the memory-side K / V projections of all decoder layers, which do not depend on the decoder state.
int tuber_linear_f32_batched(const float* x, long ldx, const float* add, long ldadd, int add_cols, const float* W, long ldw, const float* bias,
                             float* y, long ldy, int M, int N, int K, int act, int nbatch, long w_stride, long bias_stride, long y_stride,
                             hipStream_t stream) {
    return linear_f32_launch(x, ldx, add, ldadd, add_cols, W, ldw, bias, y, ldy, M, N, K, act, nbatch, w_stride, bias_stride, y_stride, stream);
}

static int attention_f32_launch(const float* q, RowMap mq, const float* k, RowMap mk, const float* v, RowMap mv, float* o, RowMap mo, const void* kpm,
                                int B, int H, int Lq, int Lk, float scale, hipStream_t stream) {
    // queries per workgroup: 32 when there are more than 16 and their score rows fit into the 160 KB of LDS beside the fixed part, else 16
    auto lds_bytes = [&](int qcap) { return (size_t)(qcap * 32 + qcap + 8 * qcap * 32 + (long)qcap * Lk) * sizeof(float); };
    const int QCAP = Lq > 16 && lds_bytes(32) <= 160 * 1024 ? 32 : 16;
    const size_t lds = lds_bytes(QCAP);
    if (lds > 160 * 1024) return TUBER_EINVAL;                      // Lk > ~2 250 keys: not a shape of this model
    if (lds > 48 * 1024) {                                          // one-time opt-in per kernel and device (the library's pattern: common.h)
        static LdsOptIn opt[2];
        if (QCAP == 32) TUBER_LDS_OPT_IN(opt[1], attention_f32_kernel<32>, 160 * 1024);
        else TUBER_LDS_OPT_IN(opt[0], attention_f32_kernel<16>, 160 * 1024);
    }
    const dim3 grid(B * H * ceil_div(Lq, QCAP));
    if (QCAP == 32)
        hipLaunchKernelGGL(attention_f32_kernel<32>, grid, dim3(256), lds, stream, q, mq, k, mk, v, mv, o, mo, (const uint8_t*)kpm, H, Lq, Lk, scale);
    else
        hipLaunchKernelGGL(attention_f32_kernel<16>, grid, dim3(256), lds, stream, q, mq, k, mk, v, mv, o, mo, (const uint8_t*)kpm, H, Lq, Lk, scale);
    TUBER_RETURN_LAUNCH();
}

// fp32 multi-head attention core, head dimension 32 (nn.MultiheadAttention of the DETR decoder, transformer.py:218-240): q rows (b, i),
// k / v rows (b, j), heads side by side in the columns; kpm [B][Lk] bytes (non-zero = padded key) or NULL; o rows (b, i).
int tuber_attention_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* o, long ldo, const void* kpm,
                        int B, int H, int Lq, int Lk, float scale, hipStream_t stream) {
    if (!q || !k || !v || !o || B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0 || (ldq & 3) || (ldk & 3) || (ldv & 3)) return TUBER_EINVAL;
    return attention_f32_launch(q, RowMap{ldq, 1, Lq, 0, 1}, k, RowMap{ldk, 1, Lk, 0, 1}, v, RowMap{ldv, 1, Lk, 0, 1}, o, RowMap{ldo, 1, Lq, 0, 1}, kpm,
                                B, H, Lq, Lk, scale, stream);
}

// the same core with every operand read in place through a token map {ld, sL, s1, s2, B2} (tuber_attn_fwd's convention, 5 longs each): token l of
// sequence b is row l * sL + (b / B2) * s1 + (b % B2) * s2.  The class branch's three attentions: t (sequence over hw, batch (b, t)),
// s (sequence over t at stride hw, batch (b, hw)) and the cross-attention, whose K / V maps have s1 = 0 (stride 0 over the decoder layer).
// There is NO key padding mask (the class branch has none).  Lq, Lk <= 8: one thread per (b, query, head); otherwise the shared-score kernel.
int tuber_attention_f32_mapped(const float* q, const long* mq, const float* k, const long* mk, const float* v, const long* mv, float* o, const long* mo,
                               int B, int H, int Lq, int Lk, float scale, hipStream_t stream) {
    if (!q || !k || !v || !o || !mq || !mk || !mv || !mo || B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return TUBER_EINVAL;
    const long* ms[4] = {mq, mk, mv, mo};
    RowMap m[4];
    for (int t = 0; t < 4; ++t) {
        m[t] = RowMap{ms[t][0], ms[t][1], ms[t][2], ms[t][3], (int)ms[t][4]};
        if (m[t].ld < H * 32 || (m[t].ld & 3) || m[t].sL < 0 || m[t].s1 < 0 || m[t].s2 < 0 || m[t].B2 <= 0) return TUBER_EINVAL;
    }
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) return TUBER_EINVAL;
    if (Lq <= 8 && Lk <= 8) {
        const long n = (long)B * Lq * H;
        if (ceil_div(n, 256) > 0x7fffffff / 2) return TUBER_EINVAL;
        hipLaunchKernelGGL(attention_f32_short_kernel<8>, dim3(ceil_div(n, 256)), dim3(256), 0, stream, q, m[0], k, m[1], v, m[2], o, m[3], B, H, Lq, Lk, scale);
        TUBER_RETURN_LAUNCH();
    }
    return attention_f32_launch(q, m[0], k, m[1], v, m[2], o, m[3], nullptr, B, H, Lq, Lk, scale, stream);
}

// y = LayerNorm(x + res) with fp32 operands and outputs, each with its own leading dimension (res may be NULL); E = 256.  The class branch's
// norm1_t / norm1_s (written into the two halves of the [t | s] concatenation) and norm2 (transformer_layers.py:58-69, post-norm).
int tuber_layernorm_f32_rows(const float* x, long ldx, const float* res, long ldres, const float* gamma, const float* beta, float* y, long ldy,
                             int M, int E, float eps, hipStream_t stream) {
    if (!x || !y || !gamma || !beta || M <= 0 || E != 256 || ldx < E || ldy < E || (ldx & 3) || (ldy & 3) || (res && (ldres < E || (ldres & 3)))) return TUBER_EINVAL;
    hipLaunchKernelGGL(layernorm_f32_rows_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, stream, x, ldx, res, ldres, gamma, beta, y, ldy, M, eps);
    TUBER_RETURN_LAUNCH();
}

}  // extern "C"
