// One-channel sigmoid (binary) heads for gfx950: the reference's binary loss family (utilities/losses_2.py: FocalLoss, JaccardLoss,
// DiceLoss, BCEJaccardLoss, BCEDiceLoss, iou, f_score; utilities/pytorch_losses.py: bce_loss and the num_classes == 1 branches of
// dice_loss / jaccard_loss / tversky_loss), the sigmoid forms of softmax_mse_loss / softmax_kl_loss (utilities/losses_1.py:9-48) and the
// thresholded 2 x 2 confusion matrix.
//   uaps_binloss_fwd   one pass over the logits z [B,1,H,W]: n, P = sum p, G = sum g, I = sum g p, sum bce, sum focal and the
//                      out-of-range label count; a finalize launch forms whichever terms the mask selects and the backward's factors
//   uaps_binloss_bwd   one launch: d loss / dz in closed form from those factors
// One channel is one float per pixel, so the planes of a batch are ONE flat run of B H W floats: a lane owns four consecutive elements
// (one 16-byte load of z, one of a float target or two of int64 labels) wherever the pointers are 16-byte aligned; the count's tail
// (N % 4 elements) and everything behind a pointer that is not 16-byte aligned goes through the scalar loop of the same kernel.
// Reduction: only seven sums per thread, so neither loss_seg.hip's per-sum wave shuffles (six steps each, 42 in all: DESIGN.md 3.14 prices
// that form at 2.4x on its 21 sums) nor loss_kernels.hpp's 33 KB [32][257] tile fits; this file uses a small LDS tile: every thread
// parks its seven values, thread t adds eight conflict-free columns of sum t / 32, seven threads add the 32 column sums in a fixed
// order -- 7 LDS writes, 8 reads and two barriers per thread.  One partial row per block (at most 512 blocks: two per CU, each lane
// streams several groups), added in double in block order by the finalize launch: no float atomics, two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include "../../include/uaps_hip.h"
#include "loss_common.hpp"

namespace {
using namespace uaps::loss;
constexpr int kMaxBlocks = 512;
constexpr int kSums = 7;                       // columns of a partial row: see Acc
constexpr int kCols = 8;                       // floats of a block's partial row

struct Acc { float bce = 0.f, focal = 0.f, n = 0.f, P = 0.f, G = 0.f, I = 0.f, bad = 0.f; };

// sigmoid and softplus of one logit from ONE exponential: e = exp(-|z|), sp = log1p(e) = softplus(-|z|),
// p = sigmoid(z), q = 1 - p = sigmoid(-z) (neither formed by subtraction), pq = p (1 - p)
struct Sig { float p, q, sp, pq; };
__device__ __forceinline__ Sig sigmoid_parts(float z) {
    const float e = expf(-fabsf(z)), inv = 1.f / (1.f + e), s = e * inv;
    Sig r;
    r.p = z >= 0.f ? inv : s;
    r.q = z >= 0.f ? s : inv;
    r.sp = log1pf(e);
    r.pq = s * inv;
    return r;
}

// the target of an element: g in [0, 1] and whether the element enters the sums (a label outside {0, 1} does not)
__device__ __forceinline__ bool label_target(long long t, float& g) {
    const bool ok = t == 0 || t == 1;
    g = t == 1 ? 1.f : 0.f;
    return ok;
}

// (1 - e^{-l})^gamma and, for the backward, (1 - e^{-l})^(gamma - 1); 1 - e^{-l} = -expm1(-l) keeps its digits where l is tiny
__device__ __forceinline__ float focal_mod(float one_minus_pt, float gamma, bool square) {
    return square ? one_minus_pt * one_minus_pt : powf(one_minus_pt, gamma);
}

__device__ __forceinline__ void fwd_element(float z, float g, bool ok, const uaps_binloss_params& prm, bool want_bce, bool want_focal,
                                            bool square, Acc& a) {
    const Sig s = sigmoid_parts(z);
    const float l0 = fmaxf(z, 0.f) - z * g + s.sp;                            // F.binary_cross_entropy_with_logits, no weight
    if (want_bce) {
        const float l = prm.has_pos_weight ? (1.f - g) * z + (1.f + (prm.pos_weight - 1.f) * g) * (s.sp + fmaxf(-z, 0.f)) : l0;
        a.bce += ok ? l : 0.f;
    }
    if (want_focal) {
        const float f = focal_mod(-expm1f(-l0), prm.focal_gamma, square) * l0;
        a.focal += ok ? f : 0.f;
    }
    a.n += ok ? 1.f : 0.f;
    a.P += ok ? s.p : 0.f;
    a.G += ok ? g : 0.f;
    a.I += ok ? g * s.p : 0.f;
    a.bad += ok ? 0.f : 1.f;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// `nvec` groups of four elements, then the elements [4 nvec, N) one by one
template <bool SOFT>
__global__ __launch_bounds__(kThreads) void bin_fwd_kernel(const float* __restrict__ z, const void* __restrict__ target,
                                                           uaps_binloss_params prm, long nvec, long N, float* __restrict__ partials) {
    __shared__ float tile[kSums][kThreads + 1];
    __shared__ float part[kSums][32];
    const bool want_bce = prm.terms & UAPS_BIN_BCE, want_focal = prm.terms & UAPS_BIN_FOCAL, square = prm.focal_gamma == 2.f;
    const long stride = (long)gridDim.x * kThreads, first = (long)blockIdx.x * kThreads + threadIdx.x;
    Acc a;
    for (long i = first; i < nvec; i += stride) {
        const float4 zv = reinterpret_cast<const float4*>(z)[i];
        const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
        float g[4];
        bool ok[4] = {true, true, true, true};
        if constexpr (SOFT) {
            const float4 gv = reinterpret_cast<const float4*>(target)[i];
            g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
        } else {
            const longlong2 t0 = reinterpret_cast<const longlong2*>(target)[2 * i], t1 = reinterpret_cast<const longlong2*>(target)[2 * i + 1];
            ok[0] = label_target(t0.x, g[0]); ok[1] = label_target(t0.y, g[1]);
            ok[2] = label_target(t1.x, g[2]); ok[3] = label_target(t1.y, g[3]);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) fwd_element(zz[v], g[v], ok[v], prm, want_bce, want_focal, square, a);
    }
    for (long i = 4 * nvec + first; i < N; i += stride) {
        float g;
        bool ok = true;
        if constexpr (SOFT) g = reinterpret_cast<const float*>(target)[i];
        else ok = label_target(reinterpret_cast<const long long*>(target)[i], g);
        fwd_element(z[i], g, ok, prm, want_bce, want_focal, square, a);
    }
    // block sums through the LDS tile (see the head of this file)
    const int t = threadIdx.x;
    const float mine[kSums] = {a.bce, a.focal, a.n, a.P, a.G, a.I, a.bad};
#pragma unroll
    for (int k = 0; k < kSums; ++k) tile[k][t] = mine[k];
    __syncthreads();
    const int k = t >> 5, j = t & 31;
    if (k < kSums) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int c = 0; c < kThreads / 32; c += 2) {
            s0 += tile[k][j + 32 * c];
            s1 += tile[k][j + 32 * (c + 1)];
        }
        part[k][j] = s0 + s1;
    }
    __syncthreads();
    if (t < kSums) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 32; ++c) s += part[t][c];
        partials[(long)blockIdx.x * kCols + t] = s;
    }
}

// Column sums over the blocks in double, in block order; then the selected terms and the backward's factors (scalar layout:
// include/uaps_hip.h, UAPS_BIN_S_*).  With n, P, G, I:
//   jaccard   1 - (I + e) / U,  U = G + P - I + e:            d/dI = -(U + I + e) / U^2,   d/dP = (I + e) / U^2
//   fscore    1 - ((1 + b2) I + e) / D,  D = (1 + b2) I + b2 (G - I) + (P - I) + e  (= b2 G + P + e: the I's cancel):
//                                                              d/dI = -(1 + b2) / D,        d/dP = ((1 + b2) I + e) / D^2
//   dice2, jaccard2, tversky2: 1 - (f(I, P, G) + f(I', A', N')) / 2 with f of loss_seg.hip and the negative channel's
//             I' = n - P - G + I,  A' = n - P,  N' = n - G:    dI'/dI = 1,  dI'/dP = -1,  dA'/dP = -1
__global__ __launch_bounds__(64) void bin_finalize(const float* __restrict__ partials, int blocks, uaps_binloss_params prm,
                                                   float* __restrict__ s) {
    __shared__ double sum[kCols];
    const int t = threadIdx.x;
    column_sums<kCols>(partials, 0, blocks, kSums, sum);
    __syncthreads();
    if (t != 0) return;
    const double n = sum[2], P = sum[3], G = sum[4], I = sum[5];
    const double eps = (double)prm.eps, b2 = (double)prm.beta * (double)prm.beta;
    const double al = (double)prm.tversky_alpha, be = (double)prm.tversky_beta;
    double term[UAPS_BIN_NTERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double gP = 0.0, gI = 0.0, k_bce = 0.0, k_focal = 0.0;
    const double inv_n = n > 0.0 ? 1.0 / n : 0.0;       // no element entered (every label out of range): the means are 0, not 0 / 0
    if (prm.terms & UAPS_BIN_BCE) {
        term[0] = sum[0] * inv_n;
        k_bce = (double)prm.coef[0] * inv_n;
    }
    if (prm.terms & UAPS_BIN_FOCAL) {
        const double a = (double)prm.focal_alpha;
        term[1] = prm.focal_mean ? a * sum[1] * inv_n : a * sum[1];
        k_focal = prm.focal_mean ? (double)prm.coef[1] * a * inv_n : (double)prm.coef[1] * a;
    }
    if (prm.terms & UAPS_BIN_JACCARD) {
        const double U = G + P - I + eps, k = (double)prm.coef[2];
        term[2] = 1.0 - (I + eps) / U;
        gI -= k * (U + I + eps) / (U * U);
        gP += k * (I + eps) / (U * U);
    }
    if (prm.terms & UAPS_BIN_FSCORE) {
        const double num = (1.0 + b2) * I + eps, D = (1.0 + b2) * I + b2 * (G - I) + (P - I) + eps, k = (double)prm.coef[3];
        term[3] = 1.0 - num / D;
        gI -= k * (1.0 + b2) / D;
        gP += k * num / (D * D);
    }
    const double In = n - P - G + I, An = n - P, Nn = n - G;
    if (prm.terms & UAPS_BIN_DICE2) {
        const double dp = P + G + eps, dn = An + Nn + eps, k = 0.5 * (double)prm.coef[4];
        term[4] = 1.0 - 0.5 * (2.0 * I / dp + 2.0 * In / dn);
        const double fIp = -k * 2.0 / dp, fAp = k * 2.0 * I / (dp * dp), fIn = -k * 2.0 / dn, fAn = k * 2.0 * In / (dn * dn);
        gI += fIp + fIn;
        gP += fAp - fIn - fAn;
    }
    if (prm.terms & UAPS_BIN_JACCARD2) {
        const double dp = P + G - I + eps, dn = An + Nn - In + eps, k = 0.5 * (double)prm.coef[5];
        term[5] = 1.0 - 0.5 * (I / dp + In / dn);
        const double fIp = -k * (dp + I) / (dp * dp), fAp = k * I / (dp * dp), fIn = -k * (dn + In) / (dn * dn), fAn = k * In / (dn * dn);
        gI += fIp + fIn;
        gP += fAp - fIn - fAn;
    }
    if (prm.terms & UAPS_BIN_TVERSKY2) {
        const double dp = I + al * (P - I) + be * (G - I) + eps, dn = In + al * (An - In) + be * (Nn - In) + eps;
        const double k = 0.5 * (double)prm.coef[6];
        term[6] = 1.0 - 0.5 * (I / dp + In / dn);
        const double fIp = -k * (dp - I * (1.0 - al - be)) / (dp * dp), fAp = k * al * I / (dp * dp);
        const double fIn = -k * (dn - In * (1.0 - al - be)) / (dn * dn), fAn = k * al * In / (dn * dn);
        gI += fIp + fIn;
        gP += fAp - fIn - fAn;
    }
    double loss = 0.0;
    for (int k = 0; k < UAPS_BIN_NTERMS; ++k) {
        s[UAPS_BIN_S_TERM + k] = (float)term[k];
        if (prm.terms & (1u << k)) loss += (double)prm.coef[k] * term[k];
    }
    s[UAPS_BIN_S_LOSS] = (float)loss;
    s[UAPS_BIN_S_BAD] = (float)sum[6];
    s[UAPS_BIN_S_N] = (float)n;
    s[UAPS_BIN_S_P] = (float)P;
    s[UAPS_BIN_S_G] = (float)G;
    s[UAPS_BIN_S_I] = (float)I;
    s[UAPS_BIN_S_GP] = (float)gP;
    s[UAPS_BIN_S_GI] = (float)gI;
    s[UAPS_BIN_S_KBCE] = (float)k_bce;
    s[UAPS_BIN_S_KFOCAL] = (float)k_focal;
    for (int k = UAPS_BIN_S_KFOCAL + 1; k < UAPS_BIN_S_NSCALARS; ++k) s[k] = 0.f;
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
//   dz = grad [ k_bce ((1 + (w - 1) g) p - w g) + k_focal ((1 - pt)^gamma + gamma (1 - pt)^(gamma - 1) pt l0) (p - g) + p (1 - p) (gP + g gI) ]
// with pt = e^{-l0} carrying its gradient (losses_2.FocalLoss does not detach it); 0 at a label outside {0, 1}.
struct BwdK { float k_bce, k_focal, gP, gI, w, gamma; bool want_focal, square; };

__device__ __forceinline__ float bwd_element(float z, float g, bool ok, const BwdK& k) {
    const Sig s = sigmoid_parts(z);
    float d = k.k_bce * ((1.f + (k.w - 1.f) * g) * s.p - k.w * g) + s.pq * (k.gP + g * k.gI);
    if (k.want_focal) {
        const float l0 = fmaxf(z, 0.f) - z * g + s.sp, om = -expm1f(-l0), pt = expf(-l0);
        const float m1 = k.square ? om : (om > 0.f ? powf(om, k.gamma - 1.f) : 0.f);
        d += k.k_focal * (m1 * om + k.gamma * m1 * pt * l0) * (s.p - g);
    }
    return ok ? d : 0.f;
}

template <bool SOFT>
__global__ __launch_bounds__(kThreads) void bin_bwd_kernel(const float* __restrict__ z, const void* __restrict__ target,
                                                           uaps_binloss_params prm, const float* __restrict__ s,
                                                           const float* __restrict__ grad, long nvec, long N, float* __restrict__ dz) {
    const float gs = grad ? grad[0] : 1.f;
    BwdK k;
    k.k_bce = gs * s[UAPS_BIN_S_KBCE]; k.k_focal = gs * s[UAPS_BIN_S_KFOCAL];
    k.gP = gs * s[UAPS_BIN_S_GP]; k.gI = gs * s[UAPS_BIN_S_GI];
    k.w = prm.has_pos_weight ? prm.pos_weight : 1.f;
    k.gamma = prm.focal_gamma; k.want_focal = prm.terms & UAPS_BIN_FOCAL; k.square = prm.focal_gamma == 2.f;
    const long stride = (long)gridDim.x * kThreads, first = (long)blockIdx.x * kThreads + threadIdx.x;
    for (long i = first; i < nvec; i += stride) {
        const float4 zv = reinterpret_cast<const float4*>(z)[i];
        float g[4];
        bool ok[4] = {true, true, true, true};
        if constexpr (SOFT) {
            const float4 gv = reinterpret_cast<const float4*>(target)[i];
            g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
        } else {
            const longlong2 t0 = reinterpret_cast<const longlong2*>(target)[2 * i], t1 = reinterpret_cast<const longlong2*>(target)[2 * i + 1];
            ok[0] = label_target(t0.x, g[0]); ok[1] = label_target(t0.y, g[1]);
            ok[2] = label_target(t1.x, g[2]); ok[3] = label_target(t1.y, g[3]);
        }
        float4 o;
        o.x = bwd_element(zv.x, g[0], ok[0], k); o.y = bwd_element(zv.y, g[1], ok[1], k);
        o.z = bwd_element(zv.z, g[2], ok[2], k); o.w = bwd_element(zv.w, g[3], ok[3], k);
        reinterpret_cast<float4*>(dz)[i] = o;
    }
    for (long i = 4 * nvec + first; i < N; i += stride) {
        float g;
        bool ok = true;
        if constexpr (SOFT) g = reinterpret_cast<const float*>(target)[i];
        else ok = label_target(reinterpret_cast<const long long*>(target)[i], g);
        dz[i] = bwd_element(z[i], g, ok, k);
    }
}

// ---- the sigmoid consistency pair (utilities/losses_1.py:18-20, :38-40) -----------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sig_mse_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long nvec, long N,
                                                               float* __restrict__ out) {
    const long stride = (long)gridDim.x * kThreads, first = (long)blockIdx.x * kThreads + threadIdx.x;
    auto one = [](float x, float y) { const float d = sigmoid_parts(x).p - sigmoid_parts(y).p; return d * d; };
    for (long i = first; i < nvec; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(one(x.x, y.x), one(x.y, y.y), one(x.z, y.z), one(x.w, y.w));
    }
    for (long i = 4 * nvec + first; i < N; i += stride) out[i] = one(a[i], b[i]);
}

// da = g 2 (sigmoid(a) - sigmoid(b)) sigmoid(a) (1 - sigmoid(a)), g the incoming gradient of the map
__global__ __launch_bounds__(kThreads) void sig_mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                               const float* __restrict__ g, long nvec, long N, float* __restrict__ da) {
    const long stride = (long)gridDim.x * kThreads, first = (long)blockIdx.x * kThreads + threadIdx.x;
    auto one = [](float x, float y, float gg) { const Sig s = sigmoid_parts(x); return gg * 2.f * (s.p - sigmoid_parts(y).p) * s.pq; };
    for (long i = first; i < nvec; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i], gg = reinterpret_cast<const float4*>(g)[i];
        reinterpret_cast<float4*>(da)[i] = make_float4(one(x.x, y.x, gg.x), one(x.y, y.y, gg.y), one(x.z, y.z, gg.z), one(x.w, y.w, gg.w));
    }
    for (long i = 4 * nvec + first; i < N; i += stride) da[i] = one(a[i], b[i], g[i]);
}

// t (log t - log sigmoid(a)), t = sigmoid(b); log sigmoid(x) = -softplus(-x) = min(x, 0) - log1p(exp(-|x|)).  F.kl_div's xlogy: 0 at t = 0
__device__ __forceinline__ float sig_kl_element(float x, float y) {
    const Sig sa = sigmoid_parts(x), sb = sigmoid_parts(y);
    const float log_pa = fminf(x, 0.f) - sa.sp, log_t = fminf(y, 0.f) - sb.sp;
    return sb.p > 0.f ? sb.p * (log_t - log_pa) : 0.f;
}

__global__ __launch_bounds__(kThreads) void sig_kl_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long nvec, long N,
                                                              float* __restrict__ partials) {
    __shared__ float red[kWaves];
    const long stride = (long)gridDim.x * kThreads, first = (long)blockIdx.x * kThreads + threadIdx.x;
    float acc = 0.f;
    for (long i = first; i < nvec; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
        acc += (sig_kl_element(x.x, y.x) + sig_kl_element(x.y, y.y)) + (sig_kl_element(x.z, y.z) + sig_kl_element(x.w, y.w));
    }
    for (long i = 4 * nvec + first; i < N; i += stride) acc += sig_kl_element(a[i], b[i]);
    const float s = block_sum(acc, red);                                  // ONE sum: six shuffle steps are the cheap form here
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void sig_kl_finalize(const float* __restrict__ partials, int blocks, double inv_n, float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double acc = 0.0;
    for (int i = 0; i < blocks; ++i) acc += (double)partials[i];
    out[0] = (float)(acc * inv_n);
}

// da = -g sigmoid(b) (1 - sigmoid(a)) / N, g a device scalar (NULL = 1)
__global__ __launch_bounds__(kThreads) void sig_kl_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              const float* __restrict__ grad, float inv_n, long nvec, long N,
                                                              float* __restrict__ da) {
    const long stride = (long)gridDim.x * kThreads, first = (long)blockIdx.x * kThreads + threadIdx.x;
    const float k = -(grad ? grad[0] : 1.f) * inv_n;
    auto one = [k](float x, float y) { return k * sigmoid_parts(y).p * sigmoid_parts(x).q; };
    for (long i = first; i < nvec; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
        reinterpret_cast<float4*>(da)[i] = make_float4(one(x.x, y.x), one(x.y, y.y), one(x.z, y.z), one(x.w, y.w));
    }
    for (long i = 4 * nvec + first; i < N; i += stride) da[i] = one(a[i], b[i]);
}

// ---- thresholded confusion: counts[t][p], p = z > logit(threshold); integer counts per block, integer atomics: exact -------------------
__global__ __launch_bounds__(kThreads) void bin_confusion_kernel(const float* __restrict__ z, const long long* __restrict__ labels,
                                                                 float cut, long N, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int blk[4];
    if (threadIdx.x < 4) blk[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int c[4] = {0u, 0u, 0u, 0u};                // statically indexed below: four registers, no scratch
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < N; i += (long)gridDim.x * kThreads) {
        const long long t = labels[i];
        const bool pos = z[i] > cut;
        c[0] += (t == 0 && !pos) ? 1u : 0u;
        c[1] += (t == 0 && pos) ? 1u : 0u;
        c[2] += (t == 1 && !pos) ? 1u : 0u;
        c[3] += (t == 1 && pos) ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned int v = c[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&blk[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 4 && blk[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)blk[threadIdx.x]);
}

__global__ void zero4_kernel(unsigned long long* counts) { if (threadIdx.x < 4) counts[threadIdx.x] = 0ull; }

// the launch's grid: over the four-element groups where they exist, else over the elements
inline int grid_of(long nvec, long N) { return grid_for(nvec > 0 ? nvec : N, kMaxBlocks); }

int check_shape(int B, int H, int W, bool labels64) {
    if (B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if ((labels64 ? 8.0 : 4.0) * (double)B * H * W >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}
int check_count(long n) {
    if (n <= 0) return UAPS_EINVAL;
    if (4.0 * (double)n >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}

// the caller's record, size-versioned: this is the first version, so anything shorter is refused and what a later header appends is
// not read
int read_params(const uaps_binloss_params* in, uaps_binloss_params& out) {
    if (!in || in->struct_size < sizeof(uaps_binloss_params)) return UAPS_EINVAL;
    memcpy(&out, in, sizeof(uaps_binloss_params));
    out.struct_size = (uint32_t)sizeof(uaps_binloss_params);
    if (out.terms == 0 || (out.terms & ~UAPS_BIN_ALL)) return UAPS_EINVAL;
    return UAPS_OK;
}
constexpr size_t kWorkspaceBytes = (size_t)kMaxBlocks * kCols * sizeof(float);
static_assert(kSums <= kCols && kSums * 32 <= kThreads, "a partial row holds every sum; the tile reduction has 32 threads per sum");
static_assert(UAPS_BIN_S_KFOCAL < UAPS_BIN_S_NSCALARS, "scalar layout");
}  // namespace

extern "C" int uaps_binloss_workspace_bytes(int B, int H, int W, size_t* out) {
    if (!out) return UAPS_EINVAL;
    const int rc = check_shape(B, H, W, false);
    if (rc) return rc;
    *out = kWorkspaceBytes;
    return UAPS_OK;
}

extern "C" int uaps_binloss_fwd(const float* z, const void* target, const uaps_binloss_params* prm, int B, int H, int W, float* scalars,
                                void* workspace, size_t workspace_bytes, uaps_stream_t stream) {
    if (!z || !target || !scalars) return UAPS_EINVAL;
    uaps_binloss_params p;
    int rc = read_params(prm, p);
    if (!rc) rc = check_shape(B, H, W, !p.target_float);
    if (rc) return rc;
    if (!workspace || workspace_bytes < kWorkspaceBytes) return UAPS_EWORKSPACE;
    const long N = (long)B * H * W, nvec = (al16(z) && al16(target)) ? N / 4 : 0;
    const int grid = grid_of(nvec, N);
    hipStream_t st = (hipStream_t)stream;
    uaps::account_bytes((p.target_float ? 8.0 : 12.0) * (double)N);
    if (p.target_float)
        UAPS_LAUNCH_MAIN((bin_fwd_kernel<true>), dim3(grid), dim3(kThreads), 0, st, z, target, p, nvec, N, (float*)workspace);
    else
        UAPS_LAUNCH_MAIN((bin_fwd_kernel<false>), dim3(grid), dim3(kThreads), 0, st, z, target, p, nvec, N, (float*)workspace);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(bin_finalize, dim3(1), dim3(64), 0, st, (const float*)workspace, grid, p, scalars);
    return (int)hipGetLastError();
}

extern "C" int uaps_binloss_bwd(const float* z, const void* target, const uaps_binloss_params* prm, const float* scalars, const float* grad,
                                int B, int H, int W, float* dz, uaps_stream_t stream) {
    if (!z || !target || !scalars || !dz) return UAPS_EINVAL;
    uaps_binloss_params p;
    int rc = read_params(prm, p);
    if (!rc) rc = check_shape(B, H, W, !p.target_float);
    if (rc) return rc;
    const long N = (long)B * H * W, nvec = (al16(z) && al16(target) && al16(dz)) ? N / 4 : 0;
    const int grid = grid_of(nvec, N);
    hipStream_t st = (hipStream_t)stream;
    uaps::account_bytes((p.target_float ? 12.0 : 16.0) * (double)N);
    if (p.target_float)
        UAPS_LAUNCH_MAIN((bin_bwd_kernel<true>), dim3(grid), dim3(kThreads), 0, st, z, target, p, scalars, grad, nvec, N, dz);
    else
        UAPS_LAUNCH_MAIN((bin_bwd_kernel<false>), dim3(grid), dim3(kThreads), 0, st, z, target, p, scalars, grad, nvec, N, dz);
    return (int)hipGetLastError();
}

extern "C" int uaps_sigmoid_mse_fwd(const float* a, const float* b, long n, float* out, uaps_stream_t stream) {
    if (!a || !b || !out) return UAPS_EINVAL;
    const int rc = check_count(n);
    if (rc) return rc;
    const long nvec = (al16(a) && al16(b) && al16(out)) ? n / 4 : 0;
    uaps::account_bytes(12.0 * (double)n);
    UAPS_LAUNCH_MAIN(sig_mse_fwd_kernel, dim3(grid_of(nvec, n)), dim3(kThreads), 0, (hipStream_t)stream, a, b, nvec, n, out);
    return (int)hipGetLastError();
}

extern "C" int uaps_sigmoid_mse_bwd(const float* a, const float* b, const float* g_map, long n, float* da, uaps_stream_t stream) {
    if (!a || !b || !g_map || !da) return UAPS_EINVAL;
    const int rc = check_count(n);
    if (rc) return rc;
    const long nvec = (al16(a) && al16(b) && al16(g_map) && al16(da)) ? n / 4 : 0;
    uaps::account_bytes(16.0 * (double)n);
    UAPS_LAUNCH_MAIN(sig_mse_bwd_kernel, dim3(grid_of(nvec, n)), dim3(kThreads), 0, (hipStream_t)stream, a, b, g_map, nvec, n, da);
    return (int)hipGetLastError();
}

extern "C" int uaps_sigmoid_kl_fwd(const float* a, const float* b, long n, float* out_mean, void* workspace, size_t workspace_bytes,
                                   uaps_stream_t stream) {
    if (!a || !b || !out_mean) return UAPS_EINVAL;
    const int rc = check_count(n);
    if (rc) return rc;
    if (!workspace || workspace_bytes < kWorkspaceBytes) return UAPS_EWORKSPACE;
    const long nvec = (al16(a) && al16(b)) ? n / 4 : 0;
    const int grid = grid_of(nvec, n);
    hipStream_t st = (hipStream_t)stream;
    uaps::account_bytes(8.0 * (double)n);
    UAPS_LAUNCH_MAIN(sig_kl_fwd_kernel, dim3(grid), dim3(kThreads), 0, st, a, b, nvec, n, (float*)workspace);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(sig_kl_finalize, dim3(1), dim3(64), 0, st, (const float*)workspace, grid, 1.0 / (double)n, out_mean);
    return (int)hipGetLastError();
}

extern "C" int uaps_sigmoid_kl_bwd(const float* a, const float* b, const float* grad, long n, float* da, uaps_stream_t stream) {
    if (!a || !b || !da) return UAPS_EINVAL;
    const int rc = check_count(n);
    if (rc) return rc;
    const long nvec = (al16(a) && al16(b) && al16(da)) ? n / 4 : 0;
    uaps::account_bytes(12.0 * (double)n);
    UAPS_LAUNCH_MAIN(sig_kl_bwd_kernel, dim3(grid_of(nvec, n)), dim3(kThreads), 0, (hipStream_t)stream, a, b, grad,
                     (float)(1.0 / (double)n), nvec, n, da);
    return (int)hipGetLastError();
}

extern "C" int uaps_bin_confusion(const float* z, const int64_t* labels, int B, int H, int W, double threshold, int64_t* counts,
                                  uaps_stream_t stream) {
    if (!z || !labels || !counts) return UAPS_EINVAL;
    if (!(threshold > 0.0 && threshold < 1.0)) return UAPS_EINVAL;
    const int rc = check_shape(B, H, W, true);
    if (rc) return rc;
    const long N = (long)B * H * W;
    const float cut = (float)(log(threshold) - log1p(-threshold));      // logit(threshold), once, on the host
    hipStream_t st = (hipStream_t)stream;
    uaps::account_bytes(12.0 * (double)N);
    hipLaunchKernelGGL(zero4_kernel, dim3(1), dim3(64), 0, st, (unsigned long long*)counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    UAPS_LAUNCH_MAIN(bin_confusion_kernel, dim3(grid_for(N, kMaxBlocks)), dim3(kThreads), 0, st, z, (const long long*)labels, cut, N,
                     (unsigned long long*)counts);
    return (int)hipGetLastError();
}
