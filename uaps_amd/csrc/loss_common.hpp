// What the fused loss files (loss_seg, loss_cps, loss_ucc, loss_binary, loss_cct_dct, loss_mean_teacher, pair_ops) share; each keeps
// only its column layout, per-pixel arithmetic, finalize formulas and entry points.
//   uaps::loss    the reduction: wave shuffles, one LDS round over the block's four waves added as (r0 + r1) + (r2 + r3), one
//                 partial row per block, column sums in double in block order.  That fixed order is what makes two runs give the
//                 same bits: it lives here and nowhere else.  The dispatch on C and on V.  The rest of the launch scaffold (block
//                 size, grid rule, the 2 GiB refusal, the alignment rule of the four-pixel form) is call_common.hpp's, re-exported
//                 here.
//   uaps::pixel   per-pixel device helpers: a lane holds all C class logits of V consecutive pixels (V = 4: one float4 per class
//                 plane, V = 1 otherwise) in registers.
#pragma once
#include <math.h>
#include "call_common.hpp"

namespace uaps {
namespace loss {
// the launch scaffold is call_common.hpp's, shared with every other entry point; the loss files go on finding it here
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::al16; using uaps::al4;

// return CALL(C) for the class counts the kernels are built for
#define UAPS_BY_C(C, CALL) \
    switch (C) { case 2: return CALL(2); case 3: return CALL(3); case 4: return CALL(4); case 5: return CALL(5); \
                 case 6: return CALL(6); case 7: return CALL(7); case 8: return CALL(8); default: return UAPS_ERANGE; }
// KERNEL<C, 4> when `vec` (four pixels a lane), else KERNEL<C, 1>: the same grid, kThreads threads, the same arguments
#define UAPS_LAUNCH_V(vec, KERNEL, C, grid, stream, ...)                                                  \
    do {                                                                                                  \
        if (vec) UAPS_LAUNCH_MAIN((KERNEL<C, 4>), dim3(grid), dim3(uaps::kThreads), 0, stream, __VA_ARGS__); \
        else UAPS_LAUNCH_MAIN((KERNEL<C, 1>), dim3(grid), dim3(uaps::kThreads), 0, stream, __VA_ARGS__);  \
    } while (0)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum of v over the block, in every thread; red: kWaves floats of LDS.  (wave_sum's loop written out: called through the helper,
// the compiler orders two instructions of rot_cons_kernel differently, and every kernel here is to keep its instruction stream)
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                  // red is reused by the next sum of the block
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// A block's partial row over a caller-owned red[kWaves][KC]: put() reduces a lane value into column `col` (every thread of the block
// calls it, once per column), store() then writes the first n columns of the block's row of `partials`.
template <int KC>
struct PartialRow {
    float (&red)[kWaves][KC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __device__ __forceinline__ void put(int col, float v) const {
        v = wave_sum(v);
        if (lane == 0) red[wave][col] = v;
    }
    __device__ __forceinline__ void store(unsigned n, float* __restrict__ partials) const {
        __syncthreads();
        const unsigned t = threadIdx.x;
        if (t < n) partials[(long)blockIdx.x * KC + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
};

// The head of a finalize kernel: thread t < n adds column t of the rows [b0, b1) in double, in block order.  The caller's barrier
// follows.
template <int KC>
__device__ __forceinline__ void column_sums(const float* __restrict__ partials, int b0, int b1, int n, double* __restrict__ sum) {
    const int t = threadIdx.x;
    if (t < n) {
        double acc = 0.0;
        for (int i = b0; i < b1; ++i) acc += (double)partials[(long)i * KC + t];
        sum[t] = acc;
    }
}
}  // namespace loss

namespace pixel {
// V consecutive int64 labels (V = 4: two 16-byte loads) / V consecutive pseudo-label bytes (V = 4: one 4-byte store)
template <int V>
__device__ __forceinline__ void load_raw_labels(const long long* __restrict__ labels, long n, long long (&t)[V]) {
    if constexpr (V == 4) {
        const longlong2 t0 = *reinterpret_cast<const longlong2*>(labels + n), t1 = *reinterpret_cast<const longlong2*>(labels + n + 2);
        t[0] = t0.x; t[1] = t0.y; t[2] = t1.x; t[3] = t1.y;
    } else {
        t[0] = labels[n];
    }
}
template <int V>
__device__ __forceinline__ void store_bytes(uint8_t* __restrict__ dst, long n, const int (&am)[V]) {
    if constexpr (V == 4) *reinterpret_cast<uchar4*>(dst + n) = make_uchar4((uint8_t)am[0], (uint8_t)am[1], (uint8_t)am[2], (uint8_t)am[3]);
    else dst[n] = (uint8_t)am[0];
}

template <int C, int V>
__device__ __forceinline__ void load_logits(const float* __restrict__ z, long HW, float (&p)[C][V]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(z + (long)c * HW);
            p[c][0] = t.x; p[c][1] = t.y; p[c][2] = t.z; p[c][3] = t.w;
        } else {
            p[c][0] = z[(long)c * HW];
        }
    }
}

template <int C, int V>
__device__ __forceinline__ void store_planes(float* __restrict__ dz, long HW, const float (&g)[C][V]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (V == 4)
            *reinterpret_cast<float4*>(dz + (long)c * HW) = make_float4(g[c][0], g[c][1], g[c][2], g[c][3]);
        else
            dz[(long)c * HW] = g[c][0];
    }
}

// arg-max over the classes of every pixel, the lowest index among equal logits (strict >)
template <int C, int V>
__device__ __forceinline__ void argmax_logits(const float (&z)[C][V], int (&am)[V]) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float best = z[0][v];
        int idx = 0;
#pragma unroll
        for (int c = 1; c < C; ++c)
            if (z[c][v] > best) { best = z[c][v]; idx = c; }
        am[v] = idx;
    }
}

// z -> softmax(z) in place; lse[v] = log sum exp (z - max) and mx[v] = max, so that log_softmax(z)[c] = z[c] - mx - lse
template <int C, int V>
__device__ __forceinline__ void softmax_inplace(float (&z)[C][V], float (&mx)[V], float (&lse)[V]) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float m = z[0][v];
#pragma unroll
        for (int c = 1; c < C; ++c) m = fmaxf(m, z[c][v]);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) { z[c][v] = expf(z[c][v] - m); s += z[c][v]; }
#pragma unroll
        for (int c = 0; c < C; ++c) z[c][v] = z[c][v] / s;
        mx[v] = m;
        lse[v] = logf(s);
    }
}

// z[t][v] for a per-pixel class t (a select chain: no dynamically indexed registers); 0 when t is outside [0, C)
template <int C, int V>
__device__ __forceinline__ float pick(const float (&z)[C][V], int v, int t) {
    float r = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) r = (t == c) ? z[c][v] : r;
    return r;
}

// the ground truth of a pixel group (labelled rows only; -1 elsewhere and for a label outside [0, C)); returns how many were outside
template <int C, int V>
__device__ __forceinline__ float load_labels(const long long* __restrict__ labels, long n, bool lab, int (&y)[V]) {
    float bad = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) y[v] = -1;
    if (lab) {
        long long t[V];
        load_raw_labels<V>(labels, n, t);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const bool ok = t[v] >= 0 && t[v] < C;
            y[v] = ok ? (int)t[v] : -1;
            bad += ok ? 0.f : 1.f;
        }
    }
    return bad;
}

// One CE + Dice term of a pixel group whose logits `p` have been through softmax_inplace (mx, lse from it): t = the target class
// of every pixel (-1: none, the pixel enters A only), zt = the target class's LOGIT, picked before the softmax.
//   ce -= log_softmax(z)[t];  A[c] += p[c];  I[c] += p[c] [t = c];  N[c] += [t = c]
template <int C, int V>
__device__ __forceinline__ void term_fwd(const float (&p)[C][V], const int (&t)[V], const float (&zt)[V], const float (&mx)[V],
                                         const float (&lse)[V], float& ce, float (&A)[C], float (&I)[C], float (&N)[C]) {
#pragma unroll
    for (int v = 0; v < V; ++v)
        if (t[v] >= 0) ce -= zt[v] - mx[v] - lse[v];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int v = 0; v < V; ++v) {
            A[c] += p[c][v];
            I[c] += (t[v] == c) ? p[c][v] : 0.f;
            N[c] += (t[v] == c) ? 1.f : 0.f;
        }
}

// The gradient of w (CE + Dice) of one term at pixel v, ADDED to g: p = softmax(z) of the pixel group, t = the target class (-1:
// no CE part), a1 / a2 = the term's Dice coefficient rows (2 / (C (card + eps)), 2 I / (C (card + eps)^2)), inv_n = 1 / pixels:
//   CE:    w inv_n (p - onehot(t))
//   Dice:  d[c] = w (a2[c] - [t = c] a1[c]),  dz = p (d - <p, d>)
template <int C, int V>
__device__ __forceinline__ void term_grad_add(const float (&p)[C][V], int v, int t, float w, float inv_n, const float* __restrict__ a1,
                                              const float* __restrict__ a2, float (&g)[C]) {
    float d[C], dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        d[c] = w * a2[c] - ((t == c) ? w * a1[c] : 0.f);
        dot += p[c][v] * d[c];
    }
    const float cw = t >= 0 ? w * inv_n : 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] += p[c][v] * (d[c] - dot) + cw * (p[c][v] - ((t == c) ? 1.f : 0.f));
}
}  // namespace pixel
}  // namespace uaps
