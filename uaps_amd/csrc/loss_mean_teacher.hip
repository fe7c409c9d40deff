// Mean Teacher (MT/MT_train.py) and uncertainty-aware Mean Teacher (UAMT/UA_MT_train.py) for gfx950: the teacher's EMA update,
// the teacher's input noise and the fused consistency term with its closed-form student gradient.
//   uaps_ema_update            ema = ema * alpha + (1 - alpha) * param over n tensor pairs   update_ema_variables, :79-83
//   uaps_teacher_noise(_apply) out[r] = x[r % B] + clamp(0.1 n, -0.2, 0.2), (1 + T) B rows  UA_MT_train.py:180-181, 190-194
//   uaps_mc_consistency_fwd    mean_t softmax(mc_t) -> entropy -> mask -> masked softmax-MSE    UA_MT_train.py:194-214
//   uaps_mc_consistency_bwd    d loss / d student logits                                      (MT_train.py:199 with no mask)
// The per-pixel kernels follow pair_ops.hip: a lane owns one pixel and all C classes in registers (a class plane is contiguous,
// so lanes read consecutive floats), block partial sums plus one fixed-order double finalize (no float atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/uaps_hip.h"
#include "philox.hpp"
#include "loss_common.hpp"

namespace {
using namespace uaps::loss;
constexpr int kMaxBlocks = 1024;

// ---- EMA update: one launch over up to kEmaBatch tensors; block b handles chunk b of the flat chunk table ---------------------
constexpr int kEmaBatch = 128;
constexpr int kEmaChunk = 1024;               // elements per block (one float4 per lane)
struct EmaBatch {
    float* e[kEmaBatch]; const float* p[kEmaBatch];
    int n[kEmaBatch];
    int first[kEmaBatch + 1];                 // first chunk of tensor k; first[m] = total chunks
    int m;
};
__global__ __launch_bounds__(kThreads) void ema_kernel(EmaBatch t, float alpha, float one_minus_alpha) {
    const int b = blockIdx.x;
    int lo = 0, hi = t.m - 1;                 // the tensor whose chunk range holds b
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.first[mid] <= b) lo = mid; else hi = mid - 1; }
    float* __restrict__ e = t.e[lo];
    const float* __restrict__ p = t.p[lo];
    const long c0 = (long)(b - t.first[lo]) * kEmaChunk;
    const long n = t.n[lo], c1 = c0 + kEmaChunk < n ? c0 + kEmaChunk : n;
    // mul_(alpha) rounds first, then add_(param, alpha=1-alpha): one rounding each, written out so nothing is contracted differently
    if (((reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(p)) & 15) == 0) {
        const long v1 = c0 / 4 + (c1 - c0) / 4;
        for (long i = c0 / 4 + threadIdx.x; i < v1; i += kThreads) {
            float4 ev = reinterpret_cast<float4*>(e)[i];
            const float4 pv = reinterpret_cast<const float4*>(p)[i];
            ev.x = __fmaf_rn(one_minus_alpha, pv.x, __fmul_rn(ev.x, alpha));
            ev.y = __fmaf_rn(one_minus_alpha, pv.y, __fmul_rn(ev.y, alpha));
            ev.z = __fmaf_rn(one_minus_alpha, pv.z, __fmul_rn(ev.z, alpha));
            ev.w = __fmaf_rn(one_minus_alpha, pv.w, __fmul_rn(ev.w, alpha));
            reinterpret_cast<float4*>(e)[i] = ev;
        }
        for (long i = 4 * v1 + threadIdx.x; i < c1; i += kThreads) e[i] = __fmaf_rn(one_minus_alpha, p[i], __fmul_rn(e[i], alpha));
    } else {
        for (long i = c0 + threadIdx.x; i < c1; i += kThreads) e[i] = __fmaf_rn(one_minus_alpha, p[i], __fmul_rn(e[i], alpha));
    }
}

// ---- teacher input noise: flat element i of the (1 + T) B rows; Philox counter offset + i / 4, word i % 4 ----------------------
__device__ __forceinline__ float noise_of(float n) { return fminf(fmaxf(n * 0.1f, -0.2f), 0.2f); }   // clamp(randn * 0.1, -0.2, 0.2)

template <bool DRAW>
__global__ __launch_bounds__(kThreads) void teacher_noise_kernel(const float* __restrict__ x, const float* __restrict__ nin, long chw,
                                                                 long rows_x, long total4, long total, uint64_t seed, uint64_t offset,
                                                                 float* __restrict__ out, bool vec) {
    const long xn = rows_x * chw;
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < total4; g += (long)gridDim.x * kThreads) {
        float n[4];
        if (DRAW) {
            const uaps::U4 r = uaps::philox4x32_10(offset + (uint64_t)g, seed);
            const float2 a = uaps::gauss2(r.x, r.y), b = uaps::gauss2(r.z, r.w);
            n[0] = a.x; n[1] = a.y; n[2] = b.x; n[3] = b.y;
        } else if (vec) {
            const float4 v = reinterpret_cast<const float4*>(nin)[g];
            n[0] = v.x; n[1] = v.y; n[2] = v.z; n[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) n[q] = 4 * g + q < total ? nin[4 * g + q] : 0.f;
        }
        const long i0 = 4 * g;
        if (vec) {                             // chw % 4 == 0: the four elements share a row, 16-byte aligned
            const long xi = i0 % xn;
            const float4 xv = reinterpret_cast<const float4*>(x)[xi / 4];
            reinterpret_cast<float4*>(out)[g] = make_float4(xv.x + noise_of(n[0]), xv.y + noise_of(n[1]), xv.z + noise_of(n[2]),
                                                            xv.w + noise_of(n[3]));
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long i = i0 + q;
                if (i < total) out[i] = x[i % xn] + noise_of(n[q]);
            }
        }
    }
}

// ---- consistency ---------------------------------------------------------------------------------------------------------------
template <int C> __device__ __forceinline__ void softmax_p(const float (&z)[C], float (&p)[C]) {
    float mx = z[0];
#pragma unroll
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(z[c] - mx); s += p[c]; }
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = p[c] / s;
}

// T > 0: mc = raw teacher logits [T][B][C][H][W]; T == 0: mc = mean probabilities [B][C][H][W]; mc == nullptr: MT mode (no mask).
// partials[2 b] = sum m d, partials[2 b + 1] = sum m over the pixels of block b.
template <int C>
__global__ __launch_bounds__(kThreads) void mc_fwd_kernel(const float* __restrict__ s, const float* __restrict__ e,
                                                          const float* __restrict__ mc, int T, long HW, long N, float threshold,
                                                          uint8_t* __restrict__ mask, float* __restrict__ unc, float* __restrict__ partials) {
    __shared__ float red[kWaves];
    float acc_md = 0.f, acc_m = 0.f;
    const long plane = N * C;                         // one MC pass: B C H W floats
    const float invT = T > 0 ? 1.f / (float)T : 1.f;
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < N; n += (long)gridDim.x * kThreads) {
        const long img = n / HW, hw = n - img * HW, base = img * C * HW + hw;
        float zs[C], ze[C], p[C], q[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { zs[c] = s[base + (long)c * HW]; ze[c] = e[base + (long)c * HW]; }
        softmax_p<C>(zs, p);
        softmax_p<C>(ze, q);
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) { const float t = p[c] - q[c]; d += t * t; }
        if (mc == nullptr) { acc_md += d; continue; }
        float pb[C];
        if (T > 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) pb[c] = 0.f;
            for (int t = 0; t < T; ++t) {
                float z[C], pt[C];
#pragma unroll
                for (int c = 0; c < C; ++c) z[c] = mc[t * plane + base + (long)c * HW];
                softmax_p<C>(z, pt);
#pragma unroll
                for (int c = 0; c < C; ++c) pb[c] += pt[c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) pb[c] *= invT;
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) pb[c] = mc[base + (long)c * HW];
        }
        float u = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) u -= pb[c] * logf(pb[c] + 1e-6f);
        const bool m = u < threshold;
        mask[n] = m ? 1 : 0;
        if (unc) unc[n] = u;
        acc_md += m ? d : 0.f;
        acc_m += m ? 1.f : 0.f;
    }
    const float smd = block_sum(acc_md, red), sm = block_sum(acc_m, red);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = smd; partials[2 * blockIdx.x + 1] = sm; }
}

// out[0] = loss, out[1] = sum m d, out[2] = sum m (MT: the normaliser B C H W and out[2] = B H W)
__global__ __launch_bounds__(64) void mc_finalize(const float* __restrict__ partials, int nblk, int masked, double n_elem, double n_pix,
                                                  float* __restrict__ out) {
    double md = 0.0, m = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) { md += (double)partials[2 * i]; m += (double)partials[2 * i + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { md += __shfl_xor(md, o, 64); m += __shfl_xor(m, o, 64); }
    if (threadIdx.x == 0) {
        const float fmd = (float)md, fm = masked ? (float)m : (float)n_pix;
        out[0] = masked ? fmd / (2.f * fm + 1e-16f) : (float)(md / n_elem);
        out[1] = fmd;
        out[2] = fm;
    }
}

// ds_c = g m / norm * 2 p_c [(p_c - q_c) - sum_k p_k (p_k - q_k)];  norm = 2 sums[2] + 1e-16 (masked) or B C H W (inv_norm)
template <int C>
__global__ __launch_bounds__(kThreads) void mc_bwd_kernel(const float* __restrict__ s, const float* __restrict__ e,
                                                          const uint8_t* __restrict__ mask, const float* __restrict__ g,
                                                          const float* __restrict__ sums, float inv_norm, long HW, long N,
                                                          float* __restrict__ ds) {
    const float scale = sums ? g[0] / (2.f * sums[2] + 1e-16f) : g[0] * inv_norm;
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < N; n += (long)gridDim.x * kThreads) {
        const long img = n / HW, hw = n - img * HW, base = img * C * HW + hw;
        float zs[C], ze[C], p[C], q[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { zs[c] = s[base + (long)c * HW]; ze[c] = e[base + (long)c * HW]; }
        const float k = (mask == nullptr || mask[n]) ? scale : 0.f;
        softmax_p<C>(zs, p);
        softmax_p<C>(ze, q);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) dot += p[c] * (p[c] - q[c]);
#pragma unroll
        for (int c = 0; c < C; ++c) ds[base + (long)c * HW] = k * (2.f * p[c] * ((p[c] - q[c]) - dot));
    }
}

template <int C> int run_fwd(const float* s, const float* e, const float* mc, int T, long HW, long N, float thr, uint8_t* mask, float* unc,
                             float* partials, int grid, hipStream_t st) {
    UAPS_LAUNCH_MAIN((mc_fwd_kernel<C>), dim3(grid), dim3(kThreads), 0, st, s, e, mc, T, HW, N, thr, mask, unc, partials);
    return (int)hipGetLastError();
}
template <int C> int run_bwd(const float* s, const float* e, const uint8_t* mask, const float* g, const float* sums, float inv_norm, long HW,
                             long N, float* ds, int grid, hipStream_t st) {
    UAPS_LAUNCH_MAIN((mc_bwd_kernel<C>), dim3(grid), dim3(kThreads), 0, st, s, e, mask, g, sums, inv_norm, HW, N, ds);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int uaps_ema_update(float* const* ema_host, const float* const* param_host, const long* numel_host, int n, float alpha,
                               float one_minus_alpha, uaps_stream_t stream) {
    if (!ema_host || !param_host || !numel_host || n <= 0) return UAPS_EINVAL;
    for (int k = 0; k < n; ++k) {                     // every argument checked before the first launch
        if (!ema_host[k] || !param_host[k] || numel_host[k] <= 0) return UAPS_EINVAL;
        if (4.0 * (double)numel_host[k] >= kTooBig) return UAPS_ERANGE;
    }
    for (int base = 0; base < n; base += kEmaBatch) {
        const int m = n - base < kEmaBatch ? n - base : kEmaBatch;
        EmaBatch t{};
        t.m = m;
        long chunks = 0;
        for (int i = 0; i < m; ++i) {
            const int k = base + i;
            t.e[i] = ema_host[k]; t.p[i] = param_host[k]; t.n[i] = (int)numel_host[k];
            t.first[i] = (int)chunks;
            chunks += (numel_host[k] + kEmaChunk - 1) / kEmaChunk;
            uaps::account_bytes(12.0 * numel_host[k]);    // ema, param read; ema written
        }
        t.first[m] = (int)chunks;
        UAPS_LAUNCH_MAIN(ema_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, (hipStream_t)stream, t, alpha, one_minus_alpha);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return UAPS_OK;
}

static int teacher_noise_impl(const float* x, const float* noise, int B, int Cin, int H, int W, int T, uint64_t seed, uint64_t offset,
                              float* out, uaps_stream_t stream) {
    if (!x || !out || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || T < 0 || T > UAPS_MC_MAX_T) return UAPS_EINVAL;
    const long chw = (long)Cin * H * W, total = (long)(1 + T) * B * chw;
    if (4.0 * (double)total >= kTooBig) return UAPS_ERANGE;
    const bool vec = chw % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) |
                                       reinterpret_cast<uintptr_t>(noise)) & 15) == 0;
    const long total4 = (total + 3) / 4;
    uaps::account_bytes(4.0 * (total + (double)B * chw) + (noise ? 4.0 * total : 0.0));
    const int grid = grid_for(total4, 4096);
    if (noise)
        UAPS_LAUNCH_MAIN(teacher_noise_kernel<false>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, x, noise, chw, (long)B,
                           total4, total, seed, offset, out, vec);
    else
        UAPS_LAUNCH_MAIN(teacher_noise_kernel<true>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, x, noise, chw, (long)B,
                           total4, total, seed, offset, out, vec);
    return (int)hipGetLastError();
}

extern "C" int uaps_teacher_noise(const float* x, int B, int Cin, int H, int W, int T, uint64_t seed, uint64_t offset, float* out,
                                  uaps_stream_t stream) {
    return teacher_noise_impl(x, nullptr, B, Cin, H, W, T, seed, offset, out, stream);
}

extern "C" int uaps_teacher_noise_apply(const float* x, const float* noise, int B, int Cin, int H, int W, int T, float* out,
                                        uaps_stream_t stream) {
    if (!noise) return UAPS_EINVAL;
    return teacher_noise_impl(x, noise, B, Cin, H, W, T, 0, 0, out, stream);
}

extern "C" int uaps_mc_consistency_workspace_bytes(size_t* out) {
    if (!out) return UAPS_EINVAL;
    *out = (size_t)kMaxBlocks * 2 * sizeof(float);
    return UAPS_OK;
}

static int fwd_dispatch(int C, const float* s, const float* e, const float* mc, int T, long HW, long N, float thr, uint8_t* mask, float* unc,
                        float* partials, int grid, hipStream_t st) {
#define CALL(K) run_fwd<K>(s, e, mc, T, HW, N, thr, mask, unc, partials, grid, st)
    UAPS_BY_C(C, CALL)
#undef CALL
}

extern "C" int uaps_mc_consistency_fwd(const float* student, const float* teacher, const float* mc, int T, int B, int C, int H, int W,
                                       float threshold, uint8_t* mask, float* uncertainty, float* out3, void* workspace,
                                       size_t workspace_bytes, uaps_stream_t stream) {
    if (!student || !teacher || !out3 || B <= 0 || H <= 0 || W <= 0 || T < 0 || T > UAPS_MC_MAX_T) return UAPS_EINVAL;
    if (mc && !mask) return UAPS_EINVAL;                 // mask mode stores the mask the backward reads
    if (!mc && (T != 0 || uncertainty)) return UAPS_EINVAL;
    if (C < 2 || C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
    const long HW = (long)H * W, N = (long)B * HW;
    if (4.0 * (double)N * C * (T > 1 ? T : 1) >= kTooBig) return UAPS_ERANGE;
    if (!workspace || workspace_bytes < (size_t)kMaxBlocks * 2 * sizeof(float)) return UAPS_EWORKSPACE;
    uaps::account_bytes(4.0 * N * C * (2 + (mc ? (T > 0 ? T : 1) : 0)) + (mc ? N : 0) + (uncertainty ? 4.0 * N : 0.0));
    const int grid = grid_for(N, kMaxBlocks);
    hipStream_t st = (hipStream_t)stream;
    const int rc = fwd_dispatch(C, student, teacher, mc, T, HW, N, threshold, mask, uncertainty, (float*)workspace, grid, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mc_finalize, dim3(1), dim3(64), 0, st, (const float*)workspace, grid, mc ? 1 : 0, (double)N * C, (double)N, out3);
    return (int)hipGetLastError();
}

static int bwd_dispatch(int C, const float* s, const float* e, const uint8_t* mask, const float* g, const float* sums, float inv_norm, long HW,
                        long N, float* ds, int grid, hipStream_t st) {
#define CALL(K) run_bwd<K>(s, e, mask, g, sums, inv_norm, HW, N, ds, grid, st)
    UAPS_BY_C(C, CALL)
#undef CALL
}

extern "C" int uaps_mc_consistency_bwd(const float* student, const float* teacher, const uint8_t* mask, const float* grad, const float* out3,
                                       int B, int C, int H, int W, float* dstudent, uaps_stream_t stream) {
    if (!student || !teacher || !grad || !dstudent || B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if ((mask == nullptr) != (out3 == nullptr)) return UAPS_EINVAL;     // mask mode needs the forward's sum m, MT mode neither
    if (C < 2 || C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
    const long HW = (long)H * W, N = (long)B * HW;
    if (4.0 * (double)N * C >= kTooBig) return UAPS_ERANGE;
    uaps::account_bytes(4.0 * N * C * 3 + (mask ? N : 0));
    return bwd_dispatch(C, student, teacher, mask, grad, out3, (float)(1.0 / ((double)N * C)), HW, N, dstudent, grid_for(N, kMaxBlocks),
                        (hipStream_t)stream);
}
