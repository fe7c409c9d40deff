// The supervised loss family (utilities/pytorch_losses.py: ce_loss, dice_loss, jaccard_loss, tversky_loss; utilities/losses_1.py:
// FocalLoss, DiceLoss) for gfx950: whichever subset of the six terms is selected, over the logits z [B,C,H,W] and the labels [B,H,W].
//   uaps_segloss_fwd   one pass: per class A = sum p, I = sum p [y = c], N = #[y = c], Z = sum p^2, and the scalars sum w_y nll,
//                      sum w_y, sum a_y (1 - p_y)^gamma nll, the valid and the out-of-range pixel counts; the terms from them
//   uaps_segloss_bwd   d loss / dz in closed form from the per-class factors the forward left in `scalars`
// As in loss_cps.hip a lane owns a pixel (four consecutive pixels, one float4 per class plane, when the plane is a multiple of 4
// floats and the pointers are 16-byte aligned) with all C classes in registers: each logit is read once by the forward and once by
// the backward, nothing per-pixel is written but the gradient.  Block partial sums (wave shuffles, then one LDS round) go to the
// workspace, one row per block; one finalize launch adds them in double in a fixed order: no floating-point atomics, two runs give
// the same bits.  The parameters (term mask, coefficients, per-class weights) travel as a kernel argument.
// A pixel whose label equals ignore_index enters no term (a defined extension: the reference's region losses raise on such a label);
// a label outside [0, C) that is not ignore_index enters no term either and is counted.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include "../../include/uaps_hip.h"
#include "loss_common.hpp"

namespace {
using namespace uaps::loss;
using namespace uaps::pixel;
constexpr int kMaxBlocks = 1024;
constexpr int kCols = 40;                      // floats of a block's partial row: 5 + 4 C used (37 at C = 8)

// columns of a partial row
//   0  sum w_y nll     1  sum w_y     2  sum a_y (1 - p_y)^gamma nll     3  valid pixels     4  labels outside [0, C), not ignored
//   5 + ...  per class: A[c], I[c], N[c], Z[c]
__host__ __device__ constexpr int col_a(int C, int c) { return 5 + c; }
__host__ __device__ constexpr int col_i(int C, int c) { return 5 + C + c; }
__host__ __device__ constexpr int col_n(int C, int c) { return 5 + 2 * C + c; }
__host__ __device__ constexpr int col_z(int C, int c) { return 5 + 3 * C + c; }
__host__ __device__ constexpr int n_cols(int C) { return 5 + 4 * C; }

// the labels of a pixel group: y = the class, -1 for an ignored pixel and for a label outside [0, C); returns how many of the latter
template <int C, int V>
__device__ __forceinline__ float load_labels_ignore(const long long* __restrict__ labels, long n, long long ignore, int (&y)[V]) {
    long long t[V];
    load_raw_labels<V>(labels, n, t);
    float bad = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const bool ign = t[v] == ignore, in = t[v] >= 0 && t[v] < C;
        y[v] = (in && !ign) ? (int)t[v] : -1;
        bad += (in || ign) ? 0.f : 1.f;
    }
    return bad;
}

// w[t] for a per-pixel class t in [0, C) (a select chain over kernel-argument scalars: no dynamically indexed memory)
template <int C>
__device__ __forceinline__ float pick_w(const float (&w)[UAPS_MAX_CLASSES], int t) {
    float r = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) r = (t == c) ? w[c] : r;
    return r;
}

// (1 - p_y)^gamma with 1 - p_y formed as the sum of the OTHER classes' probabilities (no cancellation where p_y is close to 1)
template <int C, int V>
__device__ __forceinline__ float focal_factor(const float (&p)[C][V], int v, int y, float gamma, bool square) {
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) q += (y == c) ? 0.f : p[c][v];
    return square ? q * q : powf(q, gamma);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <int C, int V>
__global__ __launch_bounds__(kThreads) void seg_fwd_kernel(const float* __restrict__ z, const long long* __restrict__ labels,
                                                           uaps_segloss_params prm, long HW, long items, float* __restrict__ partials) {
    __shared__ float red[kWaves][kCols];
    const bool want_ce = prm.terms & UAPS_SEG_CE, want_focal = prm.terms & UAPS_SEG_FOCAL, want_z = prm.terms & UAPS_SEG_DICE_SQ;
    const bool square = prm.focal_gamma == 2.f;
    float ce = 0.f, ws = 0.f, fs = 0.f, nv = 0.f, bad = 0.f;
    float A[C], I[C], N[C], Z[C];
#pragma unroll
    for (int c = 0; c < C; ++c) A[c] = I[c] = N[c] = Z[c] = 0.f;
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < items; g += (long)gridDim.x * kThreads) {
        const long n = g * V, img = n / HW, hw = n - img * HW, base = img * C * HW + hw;
        float p[C][V], zy[V], mx[V], lse[V];
        int y[V];
        load_logits<C, V>(z + base, HW, p);
        bad += load_labels_ignore<C, V>(labels, n, prm.ignore_index, y);
#pragma unroll
        for (int v = 0; v < V; ++v) zy[v] = pick<C, V>(p, v, y[v]);
        softmax_inplace<C, V>(p, mx, lse);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const bool ok = y[v] >= 0;
            const float nll = ok ? -(zy[v] - mx[v] - lse[v]) : 0.f;
            nv += ok ? 1.f : 0.f;
            if (want_ce) {
                const float w = pick_w<C>(prm.class_weight, y[v]);          // 0 for y = -1
                ce += w * nll;
                ws += w;
            }
            if (want_focal) fs += pick_w<C>(prm.focal_alpha, y[v]) * focal_factor<C, V>(p, v, y[v], prm.focal_gamma, square) * nll;
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float q = y[v] >= 0 ? p[c][v] : 0.f;
                A[c] += q;
                I[c] += (y[v] == c) ? q : 0.f;
                N[c] += (y[v] == c) ? 1.f : 0.f;
                if (want_z) Z[c] += q * q;
            }
    }
    // wave sums by shuffles, one LDS round over the block's waves, one partial row per block
    const PartialRow<kCols> row{red};
    row.put(0, ce); row.put(1, ws); row.put(2, fs); row.put(3, nv); row.put(4, bad);
#pragma unroll
    for (int c = 0; c < C; ++c) { row.put(col_a(C, c), A[c]); row.put(col_i(C, c), I[c]); row.put(col_n(C, c), N[c]); row.put(col_z(C, c), Z[c]); }
    row.store(n_cols(C), partials);
}

// Column sums over the blocks in double, in block order; then per class the selected region terms' parts and the factors of the
// backward (scalar layout: include/uaps_hip.h, UAPS_SEG_S_*):  d loss / d p_c at a pixel of class y = GA_c + [y = c] GI_c + 2 p_c GZ_c
//   dice     f = 2 I / d,  d = A + N + eps:                  df/dI = 2 / d,                         df/dA = -2 I / d^2
//   jaccard  f = I / d,    d = A + N - I + eps:              df/dI = (d + I) / d^2,                 df/dA = -I / d^2
//   tversky  f = I / d,    d = I + al (A - I) + be (N - I) + eps:   df/dI = (d - I (1 - al - be)) / d^2,   df/dA = -al I / d^2
//   dice_sq  f = (2 I + s) / d,  d = Z + N + s:              df/dI = 2 / d,                         df/dZ = -(2 I + s) / d^2
// each term = const - (1 / C) sum_c [v_c] f_c, so its factors are -coef / C times the above.
template <int C>
__global__ __launch_bounds__(64) void seg_finalize(const float* __restrict__ partials, int blocks, uaps_segloss_params prm,
                                                   float* __restrict__ s) {
    __shared__ double sum[kCols];
    __shared__ double part[4][C];              // per class f_c of dice, jaccard, tversky and v_c (1 - f_c) of dice_sq
    const int t = threadIdx.x;
    column_sums<kCols>(partials, 0, blocks, n_cols(C), sum);
    __syncthreads();
    if (t < C) {
        const double A = sum[col_a(C, t)], I = sum[col_i(C, t)], N = sum[col_n(C, t)], Zs = sum[col_z(C, t)];
        const double eps = (double)prm.eps, sm = (double)prm.smooth, al = (double)prm.tversky_alpha, be = (double)prm.tversky_beta;
        const double inv_c = 1.0 / (double)C;
        double gA = 0.0, gI = 0.0, gZ = 0.0;
        part[0][t] = part[1][t] = part[2][t] = part[3][t] = 0.0;
        if (prm.terms & UAPS_SEG_DICE) {
            const double d = A + N + eps, k = (double)prm.coef[2] * inv_c;
            part[0][t] = 2.0 * I / d;
            gI -= k * 2.0 / d;
            gA += k * 2.0 * I / (d * d);
        }
        if (prm.terms & UAPS_SEG_JACCARD) {
            const double d = A + N - I + eps, k = (double)prm.coef[3] * inv_c;
            part[1][t] = I / d;
            gI -= k * (d + I) / (d * d);
            gA += k * I / (d * d);
        }
        if (prm.terms & UAPS_SEG_TVERSKY) {
            const double d = I + al * (A - I) + be * (N - I) + eps, k = (double)prm.coef[4] * inv_c;
            part[2][t] = I / d;
            gI -= k * (d - I * (1.0 - al - be)) / (d * d);
            gA += k * al * I / (d * d);
        }
        if (prm.terms & UAPS_SEG_DICE_SQ) {
            const double d = Zs + N + sm, v = (double)prm.dice_sq_weight[t], k = (double)prm.coef[5] * inv_c * v;
            part[3][t] = v * (1.0 - (2.0 * I + sm) / d);
            gI -= k * 2.0 / d;
            gZ += k * (2.0 * I + sm) / (d * d);
        }
        s[UAPS_SEG_S_A(C) + t] = (float)A;
        s[UAPS_SEG_S_I(C) + t] = (float)I;
        s[UAPS_SEG_S_N(C) + t] = (float)N;
        s[UAPS_SEG_S_Z(C) + t] = (float)Zs;
        s[UAPS_SEG_S_GA(C) + t] = (float)gA;
        s[UAPS_SEG_S_GI(C) + t] = (float)gI;
        s[UAPS_SEG_S_GZ(C) + t] = (float)gZ;
    }
    __syncthreads();
    if (t == 0) {
        double term[UAPS_SEG_NTERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double n_valid = sum[3];
        double k_ce = 0.0, k_focal = 0.0;
        if (prm.terms & UAPS_SEG_CE) {
            term[0] = sum[0] / sum[1];                                       // 0 / 0 = NaN when every pixel is ignored, as in torch
            k_ce = (double)prm.coef[0] / sum[1];
        }
        if (prm.terms & UAPS_SEG_FOCAL) {
            term[1] = prm.focal_mean ? sum[2] / n_valid : sum[2];
            k_focal = prm.focal_mean ? (double)prm.coef[1] / n_valid : (double)prm.coef[1];
        }
        for (int k = 0; k < 3; ++k)
            if (prm.terms & (UAPS_SEG_DICE << k)) {
                double d = 0.0;
                for (int c = 0; c < C; ++c) d += part[k][c];
                term[2 + k] = 1.0 - d / (double)C;
            }
        if (prm.terms & UAPS_SEG_DICE_SQ) {
            double d = 0.0;
            for (int c = 0; c < C; ++c) d += part[3][c];
            term[5] = d / (double)C;
        }
        double loss = 0.0;
        for (int k = 0; k < UAPS_SEG_NTERMS; ++k) {
            s[UAPS_SEG_S_TERM + k] = (float)term[k];
            if (prm.terms & (1u << k)) loss += (double)prm.coef[k] * term[k];
        }
        s[UAPS_SEG_S_LOSS] = (float)loss;
        s[UAPS_SEG_S_BAD] = (float)sum[4];
        s[UAPS_SEG_S_NVALID] = (float)n_valid;
        s[UAPS_SEG_S_WSUM] = (float)sum[1];
        s[UAPS_SEG_S_KCE] = (float)k_ce;
        s[UAPS_SEG_S_KFOCAL] = (float)k_focal;
        s[12] = s[13] = s[14] = s[15] = 0.f;
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// With p = softmax(z), at a valid pixel of class y:
//   region terms   g[c] = GA[c] + [y = c] GI[c] + 2 p[c] GZ[c],   dz = p (g - <p, g>)
//   CE and focal   (k_ce w_y + k_focal a_y (1 - p_y)^gamma) (p - onehot(y))          ((1 - p_y)^gamma is a constant: detached)
// all scaled by grad[0]; 0 at an ignored or out-of-range pixel.
template <int C, int V>
__global__ __launch_bounds__(kThreads) void seg_bwd_kernel(const float* __restrict__ z, const long long* __restrict__ labels,
                                                           uaps_segloss_params prm, const float* __restrict__ s,
                                                           const float* __restrict__ grad, long HW, long items, float* __restrict__ dz) {
    const bool want_ce = prm.terms & UAPS_SEG_CE, want_focal = prm.terms & UAPS_SEG_FOCAL;
    const bool square = prm.focal_gamma == 2.f;
    const float gs = grad ? grad[0] : 1.f;
    const float k_ce = gs * s[UAPS_SEG_S_KCE], k_focal = gs * s[UAPS_SEG_S_KFOCAL];
    float GA[C], GI[C], GZ2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        GA[c] = gs * s[UAPS_SEG_S_GA(C) + c];
        GI[c] = gs * s[UAPS_SEG_S_GI(C) + c];
        GZ2[c] = 2.f * gs * s[UAPS_SEG_S_GZ(C) + c];
    }
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < items; g += (long)gridDim.x * kThreads) {
        const long n = g * V, img = n / HW, hw = n - img * HW, base = img * C * HW + hw;
        float p[C][V], mx[V], lse[V];
        int y[V];
        load_logits<C, V>(z + base, HW, p);
        load_labels_ignore<C, V>(labels, n, prm.ignore_index, y);
        softmax_inplace<C, V>(p, mx, lse);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const bool ok = y[v] >= 0;
            float d[C], dot = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                d[c] = GA[c] + ((y[v] == c) ? GI[c] : 0.f) + p[c][v] * GZ2[c];
                dot += p[c][v] * d[c];
            }
            float pw = 0.f;
            if (want_ce) pw += k_ce * pick_w<C>(prm.class_weight, y[v]);
            if (want_focal) pw += k_focal * pick_w<C>(prm.focal_alpha, y[v]) * focal_factor<C, V>(p, v, y[v], prm.focal_gamma, square);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float q = p[c][v];
                p[c][v] = ok ? q * (d[c] - dot) + pw * (q - ((y[v] == c) ? 1.f : 0.f)) : 0.f;
            }
        }
        store_planes<C, V>(dz + base, HW, p);
    }
}

template <int C> int run_fwd(bool vec, const float* z, const long long* labels, const uaps_segloss_params& prm, int B, long HW,
                             float* scalars, float* partials, hipStream_t st) {
    const long items = (long)B * HW / (vec ? 4 : 1);
    const int grid = grid_for(items, kMaxBlocks);
    UAPS_LAUNCH_V(vec, seg_fwd_kernel, C, grid, st, z, labels, prm, HW, items, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((seg_finalize<C>), dim3(1), dim3(64), 0, st, (const float*)partials, grid, prm, scalars);
    return (int)hipGetLastError();
}

template <int C> int run_bwd(bool vec, const float* z, const long long* labels, const uaps_segloss_params& prm, const float* scalars,
                             const float* grad, int B, long HW, float* dz, hipStream_t st) {
    const long items = (long)B * HW / (vec ? 4 : 1);
    UAPS_LAUNCH_V(vec, seg_bwd_kernel, C, grid_for(items, kMaxBlocks), st, z, labels, prm, scalars, grad, HW, items, dz);
    return (int)hipGetLastError();
}

int check_shape(int B, int C, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if (C < 2 || C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
    if (4.0 * (double)B * C * H * W >= kTooBig || 8.0 * (double)B * H * W >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}

// the caller's record, size-versioned: this is the first version, so anything shorter is refused and what a later header appends is
// not read
int read_params(const uaps_segloss_params* in, uaps_segloss_params& out) {
    if (!in || in->struct_size < sizeof(uaps_segloss_params)) return UAPS_EINVAL;
    memcpy(&out, in, sizeof(uaps_segloss_params));
    out.struct_size = (uint32_t)sizeof(uaps_segloss_params);
    if (out.terms == 0 || (out.terms & ~UAPS_SEG_ALL)) return UAPS_EINVAL;
    return UAPS_OK;
}
constexpr size_t kWorkspaceBytes = (size_t)kMaxBlocks * kCols * sizeof(float);
static_assert(n_cols(UAPS_MAX_CLASSES) <= kCols && n_cols(UAPS_MAX_CLASSES) <= 64, "a partial row holds every column; finalize has a thread per column");
}  // namespace

extern "C" int uaps_segloss_workspace_bytes(int B, int C, int H, int W, size_t* out) {
    if (!out) return UAPS_EINVAL;
    const int rc = check_shape(B, C, H, W);
    if (rc) return rc;
    *out = kWorkspaceBytes;
    return UAPS_OK;
}

extern "C" int uaps_segloss_fwd(const float* z, const int64_t* labels, const uaps_segloss_params* prm, int B, int C, int H, int W,
                                float* scalars, void* workspace, size_t workspace_bytes, uaps_stream_t stream) {
    if (!z || !labels || !scalars) return UAPS_EINVAL;
    uaps_segloss_params p;
    int rc = read_params(prm, p);
    if (!rc) rc = check_shape(B, C, H, W);
    if (rc) return rc;
    if (!workspace || workspace_bytes < kWorkspaceBytes) return UAPS_EWORKSPACE;
    const long HW = (long)H * W;
    const bool vec = HW % 4 == 0 && al16(z) && al16(labels);
    uaps::account_bytes((4.0 * C + 8.0) * B * HW);
#define CALL(K) run_fwd<K>(vec, z, (const long long*)labels, p, B, HW, scalars, (float*)workspace, (hipStream_t)stream)
    UAPS_BY_C(C, CALL)
#undef CALL
}

extern "C" int uaps_segloss_bwd(const float* z, const int64_t* labels, const uaps_segloss_params* prm, const float* scalars,
                                const float* grad, int B, int C, int H, int W, float* dz, uaps_stream_t stream) {
    if (!z || !labels || !scalars || !dz) return UAPS_EINVAL;
    uaps_segloss_params p;
    int rc = read_params(prm, p);
    if (!rc) rc = check_shape(B, C, H, W);
    if (rc) return rc;
    const long HW = (long)H * W;
    const bool vec = HW % 4 == 0 && al16(z) && al16(labels) && al16(dz);
    uaps::account_bytes((8.0 * C + 8.0) * B * HW);
#define CALL(K) run_bwd<K>(vec, z, (const long long*)labels, p, scalars, grad, B, HW, dz, (hipStream_t)stream)
    UAPS_BY_C(C, CALL)
#undef CALL
}
