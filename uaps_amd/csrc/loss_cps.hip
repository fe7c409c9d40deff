// CPS (CPS/CPS_train.py:195-250) for gfx950: the loss block of cross pseudo supervision over the logits z1, z2 [N,C,H,W] of two
// networks, rows [0, B_lab) labelled and rows [B_lab, N) unlabelled, and its closed-form gradient.
//   uaps_cps_fwd   6 CE + 6 Dice terms: each network against the ground truth (:215-224), and against the OTHER network's arg-max on
//                  the labelled (:228-234) and on the unlabelled rows (:238-245); sup, labeled_cps and cps from them
//   uaps_cps_bwd   d(g_sup sup + g_lcps labeled_cps) / dz on the labelled rows, d(g_cps cps) / dz on the unlabelled ones, both tensors
// As in loss_cct_dct.hip a lane owns a pixel (four consecutive pixels, one float4 per class plane, when the plane is a multiple of 4
// floats and the pointers are 16-byte aligned) with all C classes of BOTH tensors in registers: each logit is read once by the
// forward and once by the backward, both softmaxes and both arg-maxes are formed once per pixel, nothing per-pixel is written but the
// optional pseudo-label bytes.  A block works on labelled pixels only or on unlabelled pixels only (blocks [0, gl) / [gl, gl + gu)),
// so the cross terms of both row sets share one set of accumulators.  Block partial sums (wave shuffles, then one LDS round) go to
// the workspace, one row per block; one finalize launch adds them in double in a fixed order: no floating-point atomics, two runs
// give the same bits.
// Pseudo-labels: the arg-max of the LOGITS, the lowest class index among equal logits (torch.argmax(softmax(z)) except where the fp32
// softmax rounds two different logits to one probability).  The backward forms them again from the logits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/uaps_hip.h"
#include "loss_common.hpp"

namespace {
using namespace uaps::loss;
using namespace uaps::pixel;
constexpr int kMaxBlocks = 512;                // per row set (labelled / unlabelled)
constexpr int kCols = 80;                      // floats of a block's partial row: 5 + 9 C used (77 at C = 8)

// columns of a partial row (m = 0, 1: the network)
//   [0, 2)       CE sum of network m against the ground truth           (labelled blocks)
//   [2, 4)       CE sum of network m against the other network's arg-max
//   4            number of ground-truth labels outside [0, C)
//   5 + ...      per class: A[m][c] = sum p_m[c]; IY[m][c] = sum p_m[c] [y = c]; IX[m][c] = sum p_m[c] [argmax_other = c];
//                NY[c] = #[y = c]; NP[m][c] = #[argmax_m = c]
__host__ __device__ constexpr int col_a(int C, int m, int c) { return 5 + m * C + c; }
__host__ __device__ constexpr int col_iy(int C, int m, int c) { return 5 + 2 * C + m * C + c; }
__host__ __device__ constexpr int col_ix(int C, int m, int c) { return 5 + 4 * C + m * C + c; }
__host__ __device__ constexpr int col_ny(int C, int c) { return 5 + 6 * C + c; }
__host__ __device__ constexpr int col_np(int C, int m, int c) { return 5 + 7 * C + m * C + c; }
__host__ __device__ constexpr int n_cols(int C) { return 5 + 9 * C; }

// where a block's lane item g lives: labelled blocks walk rows [0, B_lab), the others rows [B_lab, N)
struct Split { long HW; long items_l, items_u; int gl, gu, B_lab; };

// ---- forward ------------------------------------------------------------------------------------------------------------------
// One network's part of a pixel group: CE against the ground truth (labelled) and against the other network's arg-max, the class
// sums of its softmax.  z is overwritten by the softmax.
template <int C, int V>
__device__ __forceinline__ void fwd_one(float (&z)[C][V], const int (&y)[V], const int (&other)[V], bool lab, float& ce_y, float& ce_x,
                                        float (&A)[C], float (&IY)[C], float (&IX)[C]) {
    float zy[V], zx[V], mx[V], lse[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        zy[v] = pick<C, V>(z, v, y[v]);
        zx[v] = pick<C, V>(z, v, other[v]);
    }
    softmax_inplace<C, V>(z, mx, lse);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if (lab && y[v] >= 0 && y[v] < C) ce_y -= zy[v] - mx[v] - lse[v];
        ce_x -= zx[v] - mx[v] - lse[v];
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float p = z[c][v];
            A[c] += p;
            IY[c] += (lab && y[v] == c) ? p : 0.f;
            IX[c] += (other[v] == c) ? p : 0.f;
        }
}

template <int C, int V>
__global__ __launch_bounds__(kThreads) void cps_fwd_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                           const long long* __restrict__ labels, Split sp, uint8_t* __restrict__ pseudo1,
                                                           uint8_t* __restrict__ pseudo2, float* __restrict__ partials) {
    __shared__ float red[kWaves][kCols];
    const bool lab = (int)blockIdx.x < sp.gl;
    const long items = lab ? sp.items_l : sp.items_u;
    const long first = lab ? 0 : (long)sp.B_lab * sp.HW;          // first pixel of the row set
    const int blk = lab ? blockIdx.x : blockIdx.x - sp.gl, nblk = lab ? sp.gl : sp.gu;
    const long HW = sp.HW;
    float ce_y[2] = {0.f, 0.f}, ce_x[2] = {0.f, 0.f}, bad = 0.f;
    float A[2][C], IY[2][C], IX[2][C], NY[C], NP[2][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        NY[c] = 0.f;
#pragma unroll
        for (int m = 0; m < 2; ++m) A[m][c] = IY[m][c] = IX[m][c] = NP[m][c] = 0.f;
    }
    for (long g = (long)blk * kThreads + threadIdx.x; g < items; g += (long)nblk * kThreads) {
        const long n = first + g * V, img = n / HW, hw = n - img * HW, base = img * C * HW + hw;
        float a[C][V], b[C][V];
        load_logits<C, V>(z1 + base, HW, a);
        load_logits<C, V>(z2 + base, HW, b);
        int y[V], am1[V], am2[V];
        bad += load_labels<C, V>(labels, n, lab, y);
        argmax_logits<C, V>(a, am1);
        argmax_logits<C, V>(b, am2);
        if (pseudo1 != nullptr) store_bytes<V>(pseudo1, n, am1);
        if (pseudo2 != nullptr) store_bytes<V>(pseudo2, n, am2);
        fwd_one<C, V>(a, y, am2, lab, ce_y[0], ce_x[0], A[0], IY[0], IX[0]);
        fwd_one<C, V>(b, y, am1, lab, ce_y[1], ce_x[1], A[1], IY[1], IX[1]);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                NY[c] += (y[v] == c) ? 1.f : 0.f;
                NP[0][c] += (am1[v] == c) ? 1.f : 0.f;
                NP[1][c] += (am2[v] == c) ? 1.f : 0.f;
            }
    }
    // wave sums by shuffles, one LDS round over the block's waves, one partial row per block
    const PartialRow<kCols> row{red};
    row.put(0, ce_y[0]); row.put(1, ce_y[1]); row.put(2, ce_x[0]); row.put(3, ce_x[1]); row.put(4, bad);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        row.put(col_ny(C, c), NY[c]);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            row.put(col_a(C, m, c), A[m][c]);
            row.put(col_iy(C, m, c), IY[m][c]);
            row.put(col_ix(C, m, c), IX[m][c]);
            row.put(col_np(C, m, c), NP[m][c]);
        }
    }
    row.store(n_cols(C), partials);
}

// The six terms t (scalar layout: include/uaps_hip.h, UAPS_CPS_S_*): network m(t) = t & 1 on rows rows(t) against target tgt(t)
//   t = 0, 1: ground truth, labelled;  t = 2, 3: the other network's arg-max, labelled;  t = 4, 5: the same, unlabelled.
// Column sums over the labelled blocks and over the unlabelled blocks in double, each in block order; then per term and class
//   card = A + count, dice_t = 1 - mean_c 2 I / (card + eps), A1 = 2 / (C (card + eps)), A2 = 2 I / (C (card + eps)^2)
// (d dice_t / d p[c] at a pixel of target class k = A2[c] - [k = c] A1[c]).
template <int C>
__global__ __launch_bounds__(128) void cps_finalize(const float* __restrict__ partials, int gl, int gu, double n_l, double n_u, double eps,
                                                    float* __restrict__ s) {
    __shared__ double sum[2][kCols];
    __shared__ double dice_part[6][C];
    const int t = threadIdx.x;
    column_sums<kCols>(partials, 0, gl, n_cols(C), sum[0]);
    column_sums<kCols>(partials, gl, gl + gu, n_cols(C), sum[1]);
    __syncthreads();
    if (t < 6 * C) {
        const int term = t / C, c = t - term * C, m = term & 1, h = term >= 4;
        const double I = term < 2 ? sum[0][col_iy(C, m, c)] : sum[h][col_ix(C, m, c)];
        const double cnt = term < 2 ? sum[0][col_ny(C, c)] : sum[h][col_np(C, 1 - m, c)];
        const double card = sum[h][col_a(C, m, c)] + cnt, den = card + eps;
        dice_part[term][c] = 2.0 * I / den;
        s[UAPS_CPS_S_A1(C) + t] = (float)(2.0 / ((double)C * den));
        s[UAPS_CPS_S_A2(C) + t] = (float)(2.0 * I / ((double)C * den * den));
        s[UAPS_CPS_S_I(C) + t] = (float)I;
        s[UAPS_CPS_S_CARD(C) + t] = (float)card;
    }
    __syncthreads();
    if (t == 0) {
        double ce[6], dice[6];
        for (int term = 0; term < 6; ++term) {
            const int m = term & 1, h = term >= 4;
            ce[term] = (term < 2 ? sum[0][m] : sum[h][2 + m]) / (h ? n_u : n_l);
            double d = 0.0;
            for (int c = 0; c < C; ++c) d += dice_part[term][c];
            dice[term] = 1.0 - d / (double)C;
            s[UAPS_CPS_S_CE + term] = (float)ce[term];
            s[UAPS_CPS_S_DICE + term] = (float)dice[term];
        }
        s[UAPS_CPS_S_SUP] = (float)(0.5 * (ce[0] + dice[0]) + 0.5 * (ce[1] + dice[1]));
        s[UAPS_CPS_S_LCPS] = (float)((0.5 * ce[2] + 0.5 * dice[2]) + (0.5 * ce[3] + 0.5 * dice[3]));
        s[UAPS_CPS_S_CPS] = (float)((0.5 * ce[4] + 0.5 * dice[4]) + (0.5 * ce[5] + 0.5 * dice[5]));
        s[UAPS_CPS_S_BAD] = (float)sum[0][4];
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// One network's gradient of a pixel group, z -> dz in place.  With p = softmax(z), wy / wx the weights of the ground-truth and the
// cross term (0.5 g, wy = 0 on unlabelled rows), inv_n = 1 / (pixels of the row set):
//   CE:    w inv_n (p - onehot(target))
//   Dice:  g[c] = w (A2[c] - [target = c] A1[c]),  dz = p (g - <p, g>)
template <int C, int V>
__device__ __forceinline__ void bwd_one(float (&z)[C][V], const int (&y)[V], const int (&other)[V], float wy, float wx, float inv_n,
                                        const float* __restrict__ a1y, const float* __restrict__ a2y, const float* __restrict__ a1x,
                                        const float* __restrict__ a2x) {
    float mx[V], lse[V];
    softmax_inplace<C, V>(z, mx, lse);
    float ky1[C], ky2[C], kx1[C], kx2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { ky1[c] = wy * a1y[c]; ky2[c] = wy * a2y[c]; kx1[c] = wx * a1x[c]; kx2[c] = wx * a2x[c]; }
    const float cy = wy * inv_n, cx = wx * inv_n;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float g[C], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            g[c] = (ky2[c] - ((y[v] == c) ? ky1[c] : 0.f)) + (kx2[c] - ((other[v] == c) ? kx1[c] : 0.f));
            dot += z[c][v] * g[c];
        }
        const bool y_ok = y[v] >= 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float p = z[c][v];
            const float ce = (y_ok ? cy * (p - ((y[v] == c) ? 1.f : 0.f)) : 0.f) + cx * (p - ((other[v] == c) ? 1.f : 0.f));
            z[c][v] = p * (g[c] - dot) + ce;
        }
    }
}

template <int C, int V>
__global__ __launch_bounds__(kThreads) void cps_bwd_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                           const long long* __restrict__ labels, const float* __restrict__ s,
                                                           const float* __restrict__ g_sup, const float* __restrict__ g_lcps,
                                                           const float* __restrict__ g_cps, Split sp, float inv_nl, float inv_nu,
                                                           float* __restrict__ dz1, float* __restrict__ dz2) {
    const bool lab = (int)blockIdx.x < sp.gl;
    const long items = lab ? sp.items_l : sp.items_u;
    const long first = lab ? 0 : (long)sp.B_lab * sp.HW;
    const int blk = lab ? blockIdx.x : blockIdx.x - sp.gl, nblk = lab ? sp.gl : sp.gu;
    const long HW = sp.HW;
    const float wy = lab ? 0.5f * (g_sup ? g_sup[0] : 1.f) : 0.f;
    const float wx = 0.5f * (lab ? (g_lcps ? g_lcps[0] : 1.f) : (g_cps ? g_cps[0] : 1.f));
    const float inv_n = lab ? inv_nl : inv_nu;
    // coefficient rows of the terms this block's pixels belong to (term = 2 * kind + network)
    const float* __restrict__ a1 = s + UAPS_CPS_S_A1(C);
    const float* __restrict__ a2 = s + UAPS_CPS_S_A2(C);
    const int tx = lab ? 2 : 4;
    for (long g = (long)blk * kThreads + threadIdx.x; g < items; g += (long)nblk * kThreads) {
        const long n = first + g * V, img = n / HW, hw = n - img * HW, base = img * C * HW + hw;
        float a[C][V], b[C][V];
        load_logits<C, V>(z1 + base, HW, a);
        load_logits<C, V>(z2 + base, HW, b);
        int y[V], am1[V], am2[V];
        load_labels<C, V>(labels, n, lab, y);
        argmax_logits<C, V>(a, am1);
        argmax_logits<C, V>(b, am2);
        bwd_one<C, V>(a, y, am2, wy, wx, inv_n, a1 + 0 * C, a2 + 0 * C, a1 + tx * C, a2 + tx * C);
        bwd_one<C, V>(b, y, am1, wy, wx, inv_n, a1 + 1 * C, a2 + 1 * C, a1 + (tx + 1) * C, a2 + (tx + 1) * C);
        store_planes<C, V>(dz1 + base, HW, a);
        store_planes<C, V>(dz2 + base, HW, b);
    }
}

Split split_for(int N, int B_lab, long HW, int V) {
    Split sp{};
    sp.HW = HW;
    sp.B_lab = B_lab;
    sp.items_l = (long)B_lab * HW / V;
    sp.items_u = (long)(N - B_lab) * HW / V;
    sp.gl = grid_for(sp.items_l, kMaxBlocks);
    sp.gu = grid_for(sp.items_u, kMaxBlocks);
    return sp;
}

template <int C> int run_fwd(bool vec, const float* z1, const float* z2, const long long* labels, int N, int B_lab, long HW, double eps,
                             uint8_t* p1, uint8_t* p2, float* scalars, float* partials, hipStream_t st) {
    const Split sp = split_for(N, B_lab, HW, vec ? 4 : 1);
    UAPS_LAUNCH_V(vec, cps_fwd_kernel, C, sp.gl + sp.gu, st, z1, z2, labels, sp, p1, p2, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((cps_finalize<C>), dim3(1), dim3(128), 0, st, (const float*)partials, sp.gl, sp.gu, (double)B_lab * HW,
                       (double)(N - B_lab) * HW, eps, scalars);
    return (int)hipGetLastError();
}

template <int C> int run_bwd(bool vec, const float* z1, const float* z2, const long long* labels, const float* scalars, const float* g_sup,
                             const float* g_lcps, const float* g_cps, int N, int B_lab, long HW, float* dz1, float* dz2, hipStream_t st) {
    const Split sp = split_for(N, B_lab, HW, vec ? 4 : 1);
    const float inv_nl = (float)(1.0 / ((double)B_lab * HW)), inv_nu = (float)(1.0 / ((double)(N - B_lab) * HW));
    UAPS_LAUNCH_V(vec, cps_bwd_kernel, C, sp.gl + sp.gu, st, z1, z2, labels, scalars, g_sup, g_lcps, g_cps, sp, inv_nl, inv_nu, dz1, dz2);
    return (int)hipGetLastError();
}

// rows [0, B_lab) labelled and [B_lab, N) unlabelled, both non-empty (the reference's means over an empty row set are NaN)
int check_shape(int N, int B_lab, int C, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || B_lab < 1 || B_lab >= N) return UAPS_EINVAL;
    if (C < 2 || C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
    if (4.0 * (double)N * C * H * W >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}
constexpr size_t kWorkspaceBytes = (size_t)2 * kMaxBlocks * kCols * sizeof(float);
static_assert(n_cols(UAPS_MAX_CLASSES) <= kCols && n_cols(UAPS_MAX_CLASSES) <= 128, "a partial row holds every column; finalize has a thread per column");
}  // namespace

extern "C" int uaps_cps_workspace_bytes(int N, int B_lab, int C, int H, int W, size_t* out) {
    if (!out) return UAPS_EINVAL;
    const int rc = check_shape(N, B_lab, C, H, W);
    if (rc) return rc;
    *out = kWorkspaceBytes;
    return UAPS_OK;
}

extern "C" int uaps_cps_fwd(const float* z1, const float* z2, const int64_t* labels, int N, int B_lab, int C, int H, int W, float eps,
                            uint8_t* pseudo1, uint8_t* pseudo2, float* scalars, void* workspace, size_t workspace_bytes,
                            uaps_stream_t stream) {
    if (!z1 || !z2 || !labels || !scalars) return UAPS_EINVAL;
    const int rc = check_shape(N, B_lab, C, H, W);
    if (rc) return rc;
    if (!workspace || workspace_bytes < kWorkspaceBytes) return UAPS_EWORKSPACE;
    const long HW = (long)H * W;
    // four pixels a lane: the planes are multiples of 4 floats (then every row set starts on a multiple of 4 too)
    const bool vec = HW % 4 == 0 && al16(z1) && al16(z2) && al16(labels) && (!pseudo1 || al4(pseudo1)) && (!pseudo2 || al4(pseudo2));
    uaps::account_bytes(8.0 * N * C * HW + 8.0 * B_lab * HW + ((pseudo1 ? 1.0 : 0.0) + (pseudo2 ? 1.0 : 0.0)) * N * HW);
#define CALL(K) run_fwd<K>(vec, z1, z2, (const long long*)labels, N, B_lab, HW, (double)eps, pseudo1, pseudo2, scalars, (float*)workspace, (hipStream_t)stream)
    UAPS_BY_C(C, CALL)
#undef CALL
}

extern "C" int uaps_cps_bwd(const float* z1, const float* z2, const int64_t* labels, const float* scalars, const float* g_sup,
                            const float* g_lcps, const float* g_cps, int N, int B_lab, int C, int H, int W, float* dz1, float* dz2,
                            uaps_stream_t stream) {
    if (!z1 || !z2 || !labels || !scalars || !dz1 || !dz2) return UAPS_EINVAL;
    const int rc = check_shape(N, B_lab, C, H, W);
    if (rc) return rc;
    const long HW = (long)H * W;
    const bool vec = HW % 4 == 0 && al16(z1) && al16(z2) && al16(labels) && al16(dz1) && al16(dz2);
    uaps::account_bytes(16.0 * N * C * HW + 8.0 * B_lab * HW);
#define CALL(K) run_bwd<K>(vec, z1, z2, (const long long*)labels, scalars, g_sup, g_lcps, g_cps, N, B_lab, HW, dz1, dz2, (hipStream_t)stream)
    UAPS_BY_C(C, CALL)
#undef CALL
}
