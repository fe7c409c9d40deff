// UCC (UCC/UCC_train.py:147-256) for gfx950: the step's cross-cut-mixed input batch, the loss block over the logits z1, z2
// [3B,C,H,W] of the two heads (rows [0, B) labelled, [B, 2B) weak, [2B, 3B) strong) and its closed-form gradient.
//   uaps_ucc_cutmix_batch   [mix(x_l) ; crossmix(x_wk) ; crossmix(x_st)] + the mixed labels + max|.|       cross_cutmix.py:78-123
//   uaps_ucc_fwd            4 CE + 4 Dice terms, the two KL variance means and exp(-variance) means, sup, ps_1, ps_2, ps   :186-240
//   uaps_ucc_bwd            d(g_sup sup + g_ps ps) / dz for every row of both tensors
// The loss kernels follow loss_cps.hip (the per-pixel helpers are shared: loss_common.hpp): a lane owns a pixel of image i (four
// consecutive pixels when the plane is a multiple of 4 floats and the pointers are 16-byte aligned) and walks the three row blocks
// of that pixel as three PAIRS of logit vectors -- (z1, z2) labelled, (z1_wk, z2_st) = variance_1 and head 2's pseudo-supervised
// term, (z1_st, z2_wk) = variance_2 and head 1's -- so that only two vectors are live at a time and every logit is read once by the
// forward and once by the backward.  Block partial sums (wave shuffles, one LDS round) go to the workspace, one row per block; one
// finalize launch adds them in double in a fixed order: no floating-point atomics, two runs give the same bits.
// Pseudo-labels: the arg-max of the LOGITS, the lowest class index among equal logits (the CPS rule).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/uaps_hip.h"
#include "loss_common.hpp"

namespace {
using namespace uaps::loss;
using namespace uaps::pixel;
constexpr int kMaxBlocks = 1024;
constexpr int kCols = 100;                     // floats of a block's partial row: 9 + 11 C used (97 at C = 8)

// columns of a partial row; term t: 0, 1 = head 1, 2 against the ground truth; 2 = z1_st against pseudo_1; 3 = z2_st against pseudo_2
//   [0, 4)   CE sum of term t          4   labels outside [0, C)
//   5, 6     sum v1, sum exp(-v1)      7, 8   sum v2, sum exp(-v2)
//   9 + ...  per class: A[t][c] = sum p_t[c]; I[t][c] = sum p_t[c] [target_t = c]; NY[c], NP1[c], NP2[c] = #[y / pseudo_1 / pseudo_2 = c]
__host__ __device__ constexpr int col_a(int C, int t, int c) { return 9 + t * C + c; }
__host__ __device__ constexpr int col_i(int C, int t, int c) { return 9 + 4 * C + t * C + c; }
__host__ __device__ constexpr int col_n(int C, int k, int c) { return 9 + 8 * C + k * C + c; }     // k = 0: y, 1: pseudo_1, 2: pseudo_2
__host__ __device__ constexpr int n_cols(int C) { return 9 + 11 * C; }

// ---- cut-mix --------------------------------------------------------------------------------------------------------------------
// The rectangles travel as kernel arguments: per image (y0, y1, x0, x1), an unset flag as the empty rectangle.
struct Rects { int r[2][UAPS_UCC_MAX_BATCH][4]; };

__device__ __forceinline__ bool inside(const int (&r)[4], int y, int x) { return y >= r[0] && y < r[1] && x >= r[2] && x < r[3]; }

// item g = V consecutive pixels of plane (i, c); block-stride loop.  out rows: [0, B) mixed labelled, [B, 2B) weak, [2B, 3B) strong.
template <int V>
__global__ __launch_bounds__(kThreads) void ucc_cutmix_kernel(const float* __restrict__ xl, const float* __restrict__ xwk,
                                                              const float* __restrict__ xst, const long long* __restrict__ yl, Rects rc,
                                                              int B, int Cin, int W, long HW, long items, float* __restrict__ out,
                                                              long long* __restrict__ yout, float* __restrict__ amax) {
    __shared__ float s16[16];
    const long per_plane = HW / V, n = (long)B * Cin * HW;
    float m = 0.f;
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < items; g += (long)gridDim.x * kThreads) {
        const long plane = g / per_plane, hw = (g - plane * per_plane) * V;
        const int i = (int)(plane / Cin), c = (int)(plane - (long)i * Cin), nb = (i + 1) % B;
        int y = (int)(hw / W), x = (int)(hw - (long)y * W);
        bool in1[V], in2[V], any1 = false, all1 = true, all2 = true;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            in1[v] = inside(rc.r[0][i], y, x);
            in2[v] = inside(rc.r[1][i], y, x);
            any1 |= in1[v]; all1 &= in1[v]; all2 &= in2[v];
            if (++x == W) { x = 0; ++y; }
        }
        const long own = plane * HW + hw, nbr = ((long)nb * Cin + c) * HW + hw;
        float a[V], b[V], wk[V], st[V];
#pragma unroll
        for (int v = 0; v < V; ++v) a[v] = b[v] = wk[v] = st[v] = 0.f;
        if constexpr (V == 4) {
            if (!all1) { const float4 t = *reinterpret_cast<const float4*>(xl + own); a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w; }
            if (any1) { const float4 t = *reinterpret_cast<const float4*>(xl + nbr); b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w; }
            if (!all2) {
                const float4 t = *reinterpret_cast<const float4*>(xwk + own), u = *reinterpret_cast<const float4*>(xst + own);
                wk[0] = t.x; wk[1] = t.y; wk[2] = t.z; wk[3] = t.w;
                st[0] = u.x; st[1] = u.y; st[2] = u.z; st[3] = u.w;
            }
        } else {
            if (!all1) a[0] = xl[own];
            if (any1) b[0] = xl[nbr];
            if (!all2) { wk[0] = xwk[own]; st[0] = xst[own]; }
        }
        float o0[V], o1[V], o2[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            o0[v] = in1[v] ? b[v] : a[v];
            o1[v] = in2[v] ? o0[v] : wk[v];
            o2[v] = in2[v] ? o0[v] : st[v];
            m = fmaxf(m, fmaxf(fabsf(o0[v]), fmaxf(fabsf(o1[v]), fabsf(o2[v]))));
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(out + own) = make_float4(o0[0], o0[1], o0[2], o0[3]);
            *reinterpret_cast<float4*>(out + n + own) = make_float4(o1[0], o1[1], o1[2], o1[3]);
            *reinterpret_cast<float4*>(out + 2 * n + own) = make_float4(o2[0], o2[1], o2[2], o2[3]);
        } else {
            out[own] = o0[0]; out[n + own] = o1[0]; out[2 * n + own] = o2[0];
        }
        if (c == 0) {                                      // the labels of image i: one plane
            const long lo = (long)i * HW + hw, ln = (long)nb * HW + hw;
#pragma unroll
            for (int v = 0; v < V; ++v) yout[lo + v] = in1[v] ? yl[ln + v] : yl[lo + v];
        }
    }
    if (amax != nullptr) uaps::block_amax_to(amax, m, s16);
}

// ---- the loss block: what forward and backward share -----------------------------------------------------------------------------
// (a, b) = logits of the KL pair; on return a = p = softmax(a), b = q = softmax(b), l[c] = log q[c] - log p[c] (from the logits:
// finite however small a probability is), var[v] = sum_c q l = sum_c KL(log_softmax a || softmax b)   (UCC_train.py:213, :216)
template <int C, int V>
__device__ __forceinline__ void kl_pair(float (&a)[C][V], float (&b)[C][V], float (&l)[C][V], float (&var)[V], float (&mxa)[V],
                                        float (&lsea)[V], float (&mxb)[V], float (&lseb)[V]) {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int v = 0; v < V; ++v) l[c][v] = b[c][v] - a[c][v];
    softmax_inplace<C, V>(a, mxa, lsea);
    softmax_inplace<C, V>(b, mxb, lseb);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float shift = (mxa[v] - mxb[v]) + (lsea[v] - lseb[v]);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            l[c][v] += shift;
            s += b[c][v] > 0.f ? b[c][v] * l[c][v] : 0.f;          // xlogy: a zero target probability adds nothing
        }
        var[v] = s;
    }
}

template <int V>
__device__ __forceinline__ void store_floats(float* __restrict__ dst, long n, const float (&x)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst + n) = make_float4(x[0], x[1], x[2], x[3]);
    else dst[n] = x[0];
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
template <int C, int V>
__global__ __launch_bounds__(kThreads) void ucc_fwd_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                           const long long* __restrict__ labels, int B, long HW, long items,
                                                           uint8_t* __restrict__ pseudo1, uint8_t* __restrict__ pseudo2,
                                                           float* __restrict__ var1, float* __restrict__ var2, float* __restrict__ partials) {
    __shared__ float red[kWaves][kCols];
    float ce[4] = {0.f, 0.f, 0.f, 0.f}, bad = 0.f, sv[2] = {0.f, 0.f}, se[2] = {0.f, 0.f};
    float A[4][C], I[4][C], N[3][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int t = 0; t < 4; ++t) A[t][c] = I[t][c] = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) N[k][c] = 0.f;
    }
    const long rows = (long)B * C * HW;                     // floats of one row block
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < items; g += (long)gridDim.x * kThreads) {
        const long n = g * V, img = n / HW, hw = n - img * HW, base = img * C * HW + hw;
        float a[C][V], b[C][V], mxa[V], lsea[V], mxb[V], lseb[V], zt[V];
        {   // labelled rows: both heads against the ground truth (:186-191)
            int y[V];
            bad += load_labels<C, V>(labels, n, true, y);
            load_logits<C, V>(z1 + base, HW, a);
            load_logits<C, V>(z2 + base, HW, b);
            float unused[C];
#pragma unroll
            for (int v = 0; v < V; ++v) zt[v] = pick<C, V>(a, v, y[v]);
            softmax_inplace<C, V>(a, mxa, lsea);
            term_fwd<C, V>(a, y, zt, mxa, lsea, ce[0], A[0], I[0], N[0]);
#pragma unroll
            for (int v = 0; v < V; ++v) zt[v] = pick<C, V>(b, v, y[v]);
            softmax_inplace<C, V>(b, mxb, lseb);
#pragma unroll
            for (int c = 0; c < C; ++c) unused[c] = 0.f;
            term_fwd<C, V>(b, y, zt, mxb, lseb, ce[1], A[1], I[1], unused);
        }
        float l[C][V], var[V];
        int am[V];
        {   // (z1_wk, z2_st): variance_1 (:213); pseudo_2 = arg-max z1_wk (:225); term 3 = z2_st against pseudo_2 (:234)
            load_logits<C, V>(z1 + rows + base, HW, a);
            load_logits<C, V>(z2 + 2 * rows + base, HW, b);
            argmax_logits<C, V>(a, am);
            if (pseudo2 != nullptr) store_bytes<V>(pseudo2, n, am);
#pragma unroll
            for (int v = 0; v < V; ++v) zt[v] = pick<C, V>(b, v, am[v]);
            kl_pair<C, V>(a, b, l, var, mxa, lsea, mxb, lseb);
            if (var1 != nullptr) store_floats<V>(var1, n, var);
#pragma unroll
            for (int v = 0; v < V; ++v) { sv[0] += var[v]; se[0] += expf(-var[v]); }
            term_fwd<C, V>(b, am, zt, mxb, lseb, ce[3], A[3], I[3], N[2]);
        }
        {   // (z1_st, z2_wk): variance_2 (:216); pseudo_1 = arg-max z2_wk (:224); term 2 = z1_st against pseudo_1 (:233)
            load_logits<C, V>(z1 + 2 * rows + base, HW, a);
            load_logits<C, V>(z2 + rows + base, HW, b);
            argmax_logits<C, V>(b, am);
            if (pseudo1 != nullptr) store_bytes<V>(pseudo1, n, am);
#pragma unroll
            for (int v = 0; v < V; ++v) zt[v] = pick<C, V>(a, v, am[v]);
            kl_pair<C, V>(a, b, l, var, mxa, lsea, mxb, lseb);
            if (var2 != nullptr) store_floats<V>(var2, n, var);
#pragma unroll
            for (int v = 0; v < V; ++v) { sv[1] += var[v]; se[1] += expf(-var[v]); }
            term_fwd<C, V>(a, am, zt, mxa, lsea, ce[2], A[2], I[2], N[1]);
        }
    }
    // wave sums by shuffles, one LDS round over the block's waves, one partial row per block
    const PartialRow<kCols> row{red};
    row.put(0, ce[0]); row.put(1, ce[1]); row.put(2, ce[2]); row.put(3, ce[3]); row.put(4, bad);
    row.put(5, sv[0]); row.put(6, se[0]); row.put(7, sv[1]); row.put(8, se[1]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int t = 0; t < 4; ++t) { row.put(col_a(C, t, c), A[t][c]); row.put(col_i(C, t, c), I[t][c]); }
#pragma unroll
        for (int k = 0; k < 3; ++k) row.put(col_n(C, k, c), N[k][c]);
    }
    row.store(n_cols(C), partials);
}

// Column sums over the blocks in double, in block order; then per term and class (scalar layout: include/uaps_hip.h, UAPS_UCC_S_*)
//   card = A + count, dice_t = 1 - mean_c 2 I / (card + eps), A1 = 2 / (C (card + eps)), A2 = 2 I / (C (card + eps)^2)
template <int C>
__global__ __launch_bounds__(128) void ucc_finalize(const float* __restrict__ partials, int blocks, double n_pix, double eps,
                                                    float* __restrict__ s) {
    __shared__ double sum[kCols];
    __shared__ double dice_part[4][C];
    const int t = threadIdx.x;
    column_sums<kCols>(partials, 0, blocks, n_cols(C), sum);
    __syncthreads();
    if (t < 4 * C) {
        const int term = t / C, c = t - term * C;
        const int k = term < 2 ? 0 : (term == 2 ? 1 : 2);           // whose counts: y, pseudo_1, pseudo_2
        const double I = sum[col_i(C, term, c)];
        const double card = sum[col_a(C, term, c)] + sum[col_n(C, k, c)], den = card + eps;
        dice_part[term][c] = 2.0 * I / den;
        s[UAPS_UCC_S_A1(C) + t] = (float)(2.0 / ((double)C * den));
        s[UAPS_UCC_S_A2(C) + t] = (float)(2.0 * I / ((double)C * den * den));
        s[UAPS_UCC_S_I(C) + t] = (float)I;
        s[UAPS_UCC_S_CARD(C) + t] = (float)card;
    }
    __syncthreads();
    if (t == 0) {
        double ce[4], dice[4];
        for (int term = 0; term < 4; ++term) {
            ce[term] = sum[term] / n_pix;
            double d = 0.0;
            for (int c = 0; c < C; ++c) d += dice_part[term][c];
            dice[term] = 1.0 - d / (double)C;
            s[UAPS_UCC_S_CE + term] = (float)ce[term];
            s[UAPS_UCC_S_DICE + term] = (float)dice[term];
        }
        const double V1 = sum[5] / n_pix, E1 = sum[6] / n_pix, V2 = sum[7] / n_pix, E2 = sum[8] / n_pix;
        const double ps1 = 0.5 * (ce[2] + dice[2]) * E1 + V1, ps2 = 0.5 * (ce[3] + dice[3]) * E2 + V2;
        s[UAPS_UCC_S_SUP] = (float)(0.5 * (ce[0] + dice[0]) + 0.5 * (ce[1] + dice[1]));
        s[UAPS_UCC_S_PS] = (float)(ps1 + ps2);
        s[UAPS_UCC_S_PS1] = (float)ps1;
        s[UAPS_UCC_S_PS2] = (float)ps2;
        s[UAPS_UCC_S_V1] = (float)V1;
        s[UAPS_UCC_S_E1] = (float)E1;
        s[UAPS_UCC_S_V2] = (float)V2;
        s[UAPS_UCC_S_E2] = (float)E2;
        s[UAPS_UCC_S_BAD] = (float)sum[4];
        s[UAPS_UCC_S_BAD + 1] = s[UAPS_UCC_S_BAD + 2] = s[UAPS_UCC_S_BAD + 3] = 0.f;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// With M = B H W, S1 = 0.5 (ce_2 + dice_2), S2 = 0.5 (ce_3 + dice_3) and, per pixel, k1 = g_ps (1 - S1 exp(-v1)) / M, k2 likewise:
//   dz1_wk = k1 (p - q)                                   p = softmax z1_wk, q = softmax z2_st, l = log q - log p
//   dz2_st = k1 q (l - v1) + g_ps E2 dS2/dz2_st
//   dz1_st = k2 (p' - q') + g_ps E1 dS1/dz1_st            p' = softmax z1_st, q' = softmax z2_wk
//   dz2_wk = k2 q' (l' - v2)
// and 0.5 g_sup d(CE + Dice)/dz on the labelled rows.
template <int C, int V>
__global__ __launch_bounds__(kThreads) void ucc_bwd_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                           const long long* __restrict__ labels, const float* __restrict__ s,
                                                           const float* __restrict__ g_sup, const float* __restrict__ g_ps, int B, long HW,
                                                           long items, float inv_n, float* __restrict__ dz1, float* __restrict__ dz2) {
    const float gs = g_sup ? g_sup[0] : 1.f, gp = g_ps ? g_ps[0] : 1.f;
    const float* __restrict__ a1 = s + UAPS_UCC_S_A1(C);
    const float* __restrict__ a2 = s + UAPS_UCC_S_A2(C);
    const float S1 = 0.5f * (s[UAPS_UCC_S_CE + 2] + s[UAPS_UCC_S_DICE + 2]), S2 = 0.5f * (s[UAPS_UCC_S_CE + 3] + s[UAPS_UCC_S_DICE + 3]);
    const float w_sup = 0.5f * gs, w1 = 0.5f * gp * s[UAPS_UCC_S_E1], w2 = 0.5f * gp * s[UAPS_UCC_S_E2];
    const long rows = (long)B * C * HW;
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < items; g += (long)gridDim.x * kThreads) {
        const long n = g * V, img = n / HW, hw = n - img * HW, base = img * C * HW + hw;
        float a[C][V], b[C][V], mxa[V], lsea[V], mxb[V], lseb[V];
        {
            int y[V];
            load_labels<C, V>(labels, n, true, y);
            load_logits<C, V>(z1 + base, HW, a);
            load_logits<C, V>(z2 + base, HW, b);
            softmax_inplace<C, V>(a, mxa, lsea);
            softmax_inplace<C, V>(b, mxb, lseb);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float ga[C], gb[C];
#pragma unroll
                for (int c = 0; c < C; ++c) ga[c] = gb[c] = 0.f;
                term_grad_add<C, V>(a, v, y[v], w_sup, inv_n, a1 + 0 * C, a2 + 0 * C, ga);
                term_grad_add<C, V>(b, v, y[v], w_sup, inv_n, a1 + 1 * C, a2 + 1 * C, gb);
#pragma unroll
                for (int c = 0; c < C; ++c) { a[c][v] = ga[c]; b[c][v] = gb[c]; }
            }
            store_planes<C, V>(dz1 + base, HW, a);
            store_planes<C, V>(dz2 + base, HW, b);
        }
        float l[C][V], var[V];
        int am[V];
        {   // (z1_wk, z2_st)
            load_logits<C, V>(z1 + rows + base, HW, a);
            load_logits<C, V>(z2 + 2 * rows + base, HW, b);
            argmax_logits<C, V>(a, am);                                                   // pseudo_2
            kl_pair<C, V>(a, b, l, var, mxa, lsea, mxb, lseb);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float k = gp * (1.f - S1 * expf(-var[v])) * inv_n;
                float gb[C];
#pragma unroll
                for (int c = 0; c < C; ++c) gb[c] = k * b[c][v] * (l[c][v] - var[v]);
                term_grad_add<C, V>(b, v, am[v], w2, inv_n, a1 + 3 * C, a2 + 3 * C, gb);
#pragma unroll
                for (int c = 0; c < C; ++c) { a[c][v] = k * (a[c][v] - b[c][v]); b[c][v] = gb[c]; }
            }
            store_planes<C, V>(dz1 + rows + base, HW, a);
            store_planes<C, V>(dz2 + 2 * rows + base, HW, b);
        }
        {   // (z1_st, z2_wk)
            load_logits<C, V>(z1 + 2 * rows + base, HW, a);
            load_logits<C, V>(z2 + rows + base, HW, b);
            argmax_logits<C, V>(b, am);                                                   // pseudo_1
            kl_pair<C, V>(a, b, l, var, mxa, lsea, mxb, lseb);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float k = gp * (1.f - S2 * expf(-var[v])) * inv_n;
                float ga[C];
#pragma unroll
                for (int c = 0; c < C; ++c) ga[c] = k * (a[c][v] - b[c][v]);
                term_grad_add<C, V>(a, v, am[v], w1, inv_n, a1 + 2 * C, a2 + 2 * C, ga);
#pragma unroll
                for (int c = 0; c < C; ++c) { b[c][v] = k * b[c][v] * (l[c][v] - var[v]); a[c][v] = ga[c]; }
            }
            store_planes<C, V>(dz1 + 2 * rows + base, HW, a);
            store_planes<C, V>(dz2 + rows + base, HW, b);
        }
    }
}

template <int C> int run_fwd(bool vec, const float* z1, const float* z2, const long long* labels, int B, long HW, double eps, uint8_t* p1,
                             uint8_t* p2, float* v1, float* v2, float* scalars, float* partials, hipStream_t st) {
    const long items = (long)B * HW / (vec ? 4 : 1);
    const int grid = grid_for(items, kMaxBlocks);
    UAPS_LAUNCH_V(vec, ucc_fwd_kernel, C, grid, st, z1, z2, labels, B, HW, items, p1, p2, v1, v2, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((ucc_finalize<C>), dim3(1), dim3(128), 0, st, (const float*)partials, grid, (double)B * HW, eps, scalars);
    return (int)hipGetLastError();
}

template <int C> int run_bwd(bool vec, const float* z1, const float* z2, const long long* labels, const float* scalars, const float* g_sup,
                             const float* g_ps, int B, long HW, float* dz1, float* dz2, hipStream_t st) {
    const long items = (long)B * HW / (vec ? 4 : 1);
    const float inv_n = (float)(1.0 / ((double)B * HW));
    UAPS_LAUNCH_V(vec, ucc_bwd_kernel, C, grid_for(items, kMaxBlocks), st, z1, z2, labels, scalars, g_sup, g_ps, B, HW, items, inv_n, dz1, dz2);
    return (int)hipGetLastError();
}

// z1, z2: [3B, C, H, W]
int check_shape(int B, int C, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if (C < 2 || C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
    if (4.0 * 3.0 * (double)B * C * H * W >= kTooBig || 8.0 * (double)B * H * W >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}
constexpr size_t kWorkspaceBytes = (size_t)kMaxBlocks * kCols * sizeof(float);
static_assert(n_cols(UAPS_MAX_CLASSES) <= kCols && n_cols(UAPS_MAX_CLASSES) <= 128, "a partial row holds every column; finalize has a thread per column");

// flag, y0, y1, x0, x1 per image -> the kernel's rectangles (an unset flag: the empty rectangle)
int read_rects(const int32_t* list, int B, int H, int W, int (&dst)[UAPS_UCC_MAX_BATCH][4]) {
    for (int i = 0; i < B; ++i) {
        const int32_t* r = list + 5 * i;
        if (r[1] < 0 || r[2] < r[1] || r[2] > H || r[3] < 0 || r[4] < r[3] || r[4] > W) return UAPS_EINVAL;
        const bool on = r[0] != 0;
        dst[i][0] = on ? r[1] : 0; dst[i][1] = on ? r[2] : 0; dst[i][2] = on ? r[3] : 0; dst[i][3] = on ? r[4] : 0;
    }
    return UAPS_OK;
}

int cutmix_impl(float* amax, const float* x_l, const float* x_wk, const float* x_st, const int64_t* y_l, const int32_t* rects_l,
                const int32_t* rects_u, int B, int Cin, int H, int W, float* out, int64_t* y_out, uaps_stream_t stream) {
    if (!x_l || !x_wk || !x_st || !y_l || !rects_l || !rects_u || !out || !y_out || B <= 0 || Cin <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if (B > UAPS_UCC_MAX_BATCH) return UAPS_ERANGE;
    const long HW = (long)H * W, n = (long)B * Cin * HW;
    if (4.0 * 3.0 * (double)n >= kTooBig || 8.0 * (double)B * HW >= kTooBig) return UAPS_ERANGE;
    Rects rc{};
    int e = read_rects(rects_l, B, H, W, rc.r[0]);
    if (!e) e = read_rects(rects_u, B, H, W, rc.r[1]);
    if (e) return e;
    uaps::account_bytes(4.0 * 6.0 * n + 16.0 * B * HW);      // three batches read, three written; the labels read and written
    const bool vec = HW % 4 == 0 && al16(x_l) && al16(x_wk) && al16(x_st) && al16(out);
    const long items = n / (vec ? 4 : 1);
    const int grid = grid_for(items, 4096);
    if (vec)
        UAPS_LAUNCH_MAIN((ucc_cutmix_kernel<4>), dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, x_l, x_wk, x_st,
                         (const long long*)y_l, rc, B, Cin, W, HW, items, out, (long long*)y_out, amax);
    else
        UAPS_LAUNCH_MAIN((ucc_cutmix_kernel<1>), dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, x_l, x_wk, x_st,
                         (const long long*)y_l, rc, B, Cin, W, HW, items, out, (long long*)y_out, amax);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int uaps_ucc_cutmix_batch(const float* x_l, const float* x_wk, const float* x_st, const int64_t* y_l, const int32_t* rects_l,
                                     const int32_t* rects_u, int B, int Cin, int H, int W, float* out, int64_t* y_out,
                                     uaps_stream_t stream) {
    return cutmix_impl(uaps::take_hints().out_amax, x_l, x_wk, x_st, y_l, rects_l, rects_u, B, Cin, H, W, out, y_out, stream);
}
// (the *_h form: the hints of THIS call as the first argument, nothing thread-local -- see conv_fwd.hip)
extern "C" int uaps_ucc_cutmix_batch_h(const uaps_call_hints* hints, const float* x_l, const float* x_wk, const float* x_st,
                                       const int64_t* y_l, const int32_t* rects_l, const int32_t* rects_u, int B, int Cin, int H, int W,
                                       float* out, int64_t* y_out, uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    return cutmix_impl(h.out_amax, x_l, x_wk, x_st, y_l, rects_l, rects_u, B, Cin, H, W, out, y_out, stream);
}

extern "C" int uaps_ucc_workspace_bytes(int B, int C, int H, int W, size_t* out) {
    if (!out) return UAPS_EINVAL;
    const int rc = check_shape(B, C, H, W);
    if (rc) return rc;
    *out = kWorkspaceBytes;
    return UAPS_OK;
}

extern "C" int uaps_ucc_fwd(const float* z1, const float* z2, const int64_t* labels, int B, int C, int H, int W, float eps, uint8_t* pseudo1,
                            uint8_t* pseudo2, float* var1, float* var2, float* scalars, void* workspace, size_t workspace_bytes,
                            uaps_stream_t stream) {
    if (!z1 || !z2 || !labels || !scalars) return UAPS_EINVAL;
    const int rc = check_shape(B, C, H, W);
    if (rc) return rc;
    if (!workspace || workspace_bytes < kWorkspaceBytes) return UAPS_EWORKSPACE;
    const long HW = (long)H * W;
    // four pixels a lane: the planes are multiples of 4 floats (then every row block starts on a multiple of 4 too)
    const bool vec = HW % 4 == 0 && al16(z1) && al16(z2) && al16(labels) && (!pseudo1 || al4(pseudo1)) && (!pseudo2 || al4(pseudo2)) &&
                     (!var1 || al16(var1)) && (!var2 || al16(var2));
    uaps::account_bytes(24.0 * B * C * HW + 8.0 * B * HW + ((pseudo1 ? 1.0 : 0.0) + (pseudo2 ? 1.0 : 0.0)) * B * HW +
                        ((var1 ? 4.0 : 0.0) + (var2 ? 4.0 : 0.0)) * B * HW);
#define CALL(K) run_fwd<K>(vec, z1, z2, (const long long*)labels, B, HW, (double)eps, pseudo1, pseudo2, var1, var2, scalars, (float*)workspace, (hipStream_t)stream)
    UAPS_BY_C(C, CALL)
#undef CALL
}

extern "C" int uaps_ucc_bwd(const float* z1, const float* z2, const int64_t* labels, const float* scalars, const float* g_sup,
                            const float* g_ps, int B, int C, int H, int W, float* dz1, float* dz2, uaps_stream_t stream) {
    if (!z1 || !z2 || !labels || !scalars || !dz1 || !dz2) return UAPS_EINVAL;
    const int rc = check_shape(B, C, H, W);
    if (rc) return rc;
    const long HW = (long)H * W;
    const bool vec = HW % 4 == 0 && al16(z1) && al16(z2) && al16(labels) && al16(dz1) && al16(dz2);
    uaps::account_bytes(48.0 * B * C * HW + 8.0 * B * HW);
#define CALL(K) run_bwd<K>(vec, z1, z2, (const long long*)labels, scalars, g_sup, g_ps, B, HW, dz1, dz2, (hipStream_t)stream)
    UAPS_BY_C(C, CALL)
#undef CALL
}
