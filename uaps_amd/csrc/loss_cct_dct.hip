// CCT (CCT/CCT_train.py) and DCT (DCT/DCT_train.py) for gfx950: the consistency terms of the two comparison methods with their
// closed-form gradients, and the DCT step's input batch.
//   uaps_cct_consistency_fwd   (1/(D-1)) sum_k mean((softmax(z0) - softmax(zk))^2)              CCT_train.py:195-200
//   uaps_cct_consistency_bwd   d/dz of every head (both sides trained, nothing detached)
//   uaps_rot90_batch           [x_l; x_u; rot90(x_u, k, [2,3])] + max|.|                         DCT_train.py:165-175
//   uaps_rot_consistency_fwd   mean((softmax(r) - rot90(softmax(u), k))^2)                       DCT_train.py:188
//   uaps_rot_consistency_bwd   d/dr and d/du
// The CCT kernels follow loss_mean_teacher.hip: a lane owns a pixel (four consecutive pixels, one float4 per class plane, when the
// plane is a multiple of 4 floats and the pointers are 16-byte aligned) and all C classes in registers; block partial sums plus one
// fixed-order double finalize.  The rotation kernels work on 32 x 32 output tiles: the rotated operand goes through an LDS tile with
// padded rows (33 floats), so global reads and writes stay coalesced for every k, also when k is odd and the rotation transposes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/uaps_hip.h"
#include "loss_common.hpp"

namespace {
using namespace uaps::loss;
using namespace uaps::pixel;
constexpr int kMaxBlocks = 1024;
constexpr int kTile = 32;                      // output tile edge of the rotation kernels; 256 threads = 32 columns x 8 rows
constexpr int kTerms = UAPS_CCT_MAX_HEADS;     // partial sums per block (D - 1 used)

struct Heads { const float* z[UAPS_CCT_MAX_HEADS]; };
struct GradHeads { float* z[UAPS_CCT_MAX_HEADS]; };

// p[c][v] = softmax over c of the logits z[c * HW + v] (the max and the log-sum-exp of softmax_inplace are not used: dead code here)
template <int C, int V>
__device__ __forceinline__ void load_softmax(const float* __restrict__ z, long HW, float (&p)[C][V]) {
    float mx[V], lse[V];
    load_logits<C, V>(z, HW, p);
    softmax_inplace<C, V>(p, mx, lse);
}

// ---- CCT ----------------------------------------------------------------------------------------------------------------------
// groups = B H W / V lane items; off0 = b0 C H W (the window's first float); partials[blk * kTerms + k - 1] = sum over the block's
// pixels of sum_c (p0 - pk)^2.
template <int C, int V>
__global__ __launch_bounds__(kThreads) void cct_fwd_kernel(Heads h, int D, long HW, long off0, long groups, float* __restrict__ partials) {
    __shared__ float red[kWaves];
    float acc[kTerms - 1];
#pragma unroll
    for (int k = 0; k < kTerms - 1; ++k) acc[k] = 0.f;
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long)gridDim.x * kThreads) {
        const long n = g * V, img = n / HW, hw = n - img * HW, base = off0 + img * C * HW + hw;
        float p0[C][V], pk[C][V];
        load_softmax<C, V>(h.z[0] + base, HW, p0);
#pragma unroll
        for (int k = 1; k < kTerms; ++k) {
            if (k < D) {
                load_softmax<C, V>(h.z[k] + base, HW, pk);
                float d = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int v = 0; v < V; ++v) { const float t = p0[c][v] - pk[c][v]; d += t * t; }
                acc[k - 1] += d;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kTerms - 1; ++k) {
        if (k < D - 1) {                              // uniform over the block
            const float s = block_sum(acc[k], red);
            if (threadIdx.x == 0) partials[(long)blockIdx.x * kTerms + k] = s;
        }
    }
}

// out[0] = (1/(D-1)) sum_k S_k / n_elem, out[k] = S_k (k = 1..D-1), S_k summed over the blocks in double in a fixed order
__global__ __launch_bounds__(64) void cct_finalize(const float* __restrict__ partials, int nblk, int D, double n_elem, float* __restrict__ out) {
    double loss = 0.0;
    for (int k = 0; k < D - 1; ++k) {
        double s = 0.0;
        for (int i = threadIdx.x; i < nblk; i += 64) s += (double)partials[(long)i * kTerms + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (threadIdx.x == 0) out[1 + k] = (float)s;
        loss += s / n_elem;
    }
    if (threadIdx.x == 0) out[0] = (float)(loss / (double)(D - 1));
}

// L = (1/(D-1)) sum_k (1/n_elem) sum (p0 - pk)^2, a = grad[0] * 2 / ((D-1) n_elem):
//   head k >= 1: dL/dpk = -a (p0 - pk);  head 0: dL/dp0 = a sum_k (p0 - pk);  dz = p (g - <p, g>)
template <int C, int V>
__global__ __launch_bounds__(kThreads) void cct_bwd_kernel(Heads h, GradHeads dh, int D, const float* __restrict__ grad, float coef, long HW,
                                                           long off0, long groups) {
    const float a = grad[0] * coef;
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long)gridDim.x * kThreads) {
        const long n = g * V, img = n / HW, hw = n - img * HW, base = off0 + img * C * HW + hw;
        float p0[C][V], pk[C][V], s[C][V];
        load_softmax<C, V>(h.z[0] + base, HW, p0);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int v = 0; v < V; ++v) s[c][v] = 0.f;
#pragma unroll
        for (int k = 1; k < kTerms; ++k) {
            if (k < D) {
                load_softmax<C, V>(h.z[k] + base, HW, pk);
                float dot[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    dot[v] = 0.f;
#pragma unroll
                    for (int c = 0; c < C; ++c) dot[v] += pk[c][v] * (p0[c][v] - pk[c][v]);
                }
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const float diff = p0[c][v] - pk[c][v];
                        s[c][v] += diff;
                        pk[c][v] = -a * (pk[c][v] * (diff - dot[v]));
                    }
                store_planes<C, V>(dh.z[k] + base, HW, pk);
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) dot += p0[c][v] * s[c][v];
#pragma unroll
            for (int c = 0; c < C; ++c) p0[c][v] = a * (p0[c][v] * (s[c][v] - dot));
        }
        store_planes<C, V>(dh.z[0] + base, HW, p0);
    }
}

// ---- rotation geometry --------------------------------------------------------------------------------------------------------
// torch.rot90(x, k, [2, 3]) of an H x W plane is Ho x Wo (swapped for odd k) with
//   k = 0: out[i][j] = x[i][j]            k = 1: out[i][j] = x[j][W-1-i]
//   k = 2: out[i][j] = x[H-1-i][W-1-j]    k = 3: out[i][j] = x[H-1-j][i]
// The 32 x 32 output tile at (i0, j0) reads the 32 x 32 source block at (r0, c0); output (ii, jj) of the tile is source element
// (tr, tc) of the block.  Both maps are bijections between the valid parts, so guarding both sides by the plane edges suffices.
__device__ __forceinline__ void src_block(int k, int H, int W, int i0, int j0, int& r0, int& c0) {
    switch (k) {
        case 0: r0 = i0; c0 = j0; break;
        case 1: r0 = j0; c0 = W - i0 - kTile; break;
        case 2: r0 = H - i0 - kTile; c0 = W - j0 - kTile; break;
        default: r0 = H - j0 - kTile; c0 = i0; break;
    }
}
__device__ __forceinline__ void src_in_block(int k, int ii, int jj, int& tr, int& tc) {
    switch (k) {
        case 0: tr = ii; tc = jj; break;
        case 1: tr = jj; tc = kTile - 1 - ii; break;
        case 2: tr = kTile - 1 - ii; tc = kTile - 1 - jj; break;
        default: tr = kTile - 1 - jj; tc = ii; break;
    }
}

// blocks [0, cat_blocks): out[0, 2n) = [x_l ; x_u] (16-byte lanes when n4 > 0, the scalar tail in block 0);
// the others: one 32 x 32 tile of one rotated plane each, staged through LDS (read rows of the source, write rows of the output).
__global__ __launch_bounds__(kThreads) void rot90_batch_kernel(const float* __restrict__ xl, const float* __restrict__ xu, float* __restrict__ out,
                                                               float* __restrict__ rot, long n, long n4, int cat_blocks, int H, int W, int k,
                                                               int tiles_i, int tiles_j, float* __restrict__ amax) {
    __shared__ float tile[kTile][kTile + 1];
    __shared__ float s16[16];
    float m = 0.f;
    if ((int)blockIdx.x < cat_blocks) {
        for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < 2 * n4; i += (long)cat_blocks * kThreads) {
            const bool hi = i >= n4;
            const float4 v = hi ? reinterpret_cast<const float4*>(xu)[i - n4] : reinterpret_cast<const float4*>(xl)[i];
            reinterpret_cast<float4*>(out + (hi ? n : 0))[hi ? i - n4 : i] = v;
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
        if (blockIdx.x == 0)
            for (long i = 4 * n4 + threadIdx.x; i < n; i += kThreads) {
                const float a = xl[i], b = xu[i];
                out[i] = a; out[n + i] = b;
                m = fmaxf(m, fmaxf(fabsf(a), fabsf(b)));
            }
    } else {
        const int per_plane = tiles_i * tiles_j;
        const long t = (long)blockIdx.x - cat_blocks, plane = t / per_plane;
        const int ti = (int)(t - plane * per_plane) / tiles_j, tj = (int)(t - plane * per_plane) - ti * tiles_j;
        const int Ho = (k & 1) ? W : H, Wo = (k & 1) ? H : W;
        const long HW = (long)H * W;
        const float* __restrict__ src = xu + plane * HW;
        float* __restrict__ dst = rot + plane * HW;
        const int i0 = ti * kTile, j0 = tj * kTile, tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
        int r0, c0;
        src_block(k, H, W, i0, j0, r0, c0);
#pragma unroll
        for (int q = 0; q < kTile / 8; ++q) {
            const int rr = ty + 8 * q, r = r0 + rr, c = c0 + tx;
            if (r >= 0 && r < H && c >= 0 && c < W) tile[rr][tx] = src[(long)r * W + c];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kTile / 8; ++q) {
            const int ii = ty + 8 * q, i = i0 + ii, j = j0 + tx;
            if (i < Ho && j < Wo) {
                int tr, tc;
                src_in_block(k, ii, tx, tr, tc);
                const float v = tile[tr][tc];
                dst[(long)i * Wo + j] = v;
                m = fmaxf(m, fabsf(v));
            }
        }
    }
    if (amax != nullptr) uaps::block_amax_to(amax, m, s16);
}

// ---- rotation consistency -----------------------------------------------------------------------------------------------------
// r: logits of the rotated forward [*, C, Ho, Wo], u: logits of the plain forward [*, C, H, W]; r_off / u_off: first float of the
// window.  Block-stride loop over the B * tiles_i * tiles_j output tiles; u's source block of all C classes is staged in LDS.
// BWD: dr = a pr (diff - <pr, diff>), du = -a pu (diff - <pu, diff>) with diff = pr - pu, a = grad[0] * 2 / n_elem; du is written
// into the same LDS tile (each element is read by exactly one lane) and stored back in source order.
template <int C, bool BWD>
__global__ __launch_bounds__(kThreads) void rot_cons_kernel(const float* __restrict__ r, const float* __restrict__ u, long r_off, long u_off,
                                                            int B, int H, int W, int k, int tiles_i, int tiles_j, const float* __restrict__ grad,
                                                            float coef, float* __restrict__ dr, float* __restrict__ du, float* __restrict__ partials) {
    __shared__ float tile[C][kTile][kTile + 1];
    __shared__ float red[kWaves];
    const int Ho = (k & 1) ? W : H, Wo = (k & 1) ? H : W;
    const long HW = (long)H * W;
    const int per_img = tiles_i * tiles_j;
    const long total = (long)B * per_img;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const float a = BWD ? grad[0] * coef : 0.f;
    float acc = 0.f;
    for (long t = blockIdx.x; t < total; t += gridDim.x) {
        const long b = t / per_img;
        const int ti = (int)(t - b * per_img) / tiles_j, tj = (int)(t - b * per_img) - ti * tiles_j;
        const int i0 = ti * kTile, j0 = tj * kTile;
        const float* __restrict__ ub = u + u_off + b * C * HW;
        const float* __restrict__ rb = r + r_off + b * C * HW;
        int r0, c0;
        src_block(k, H, W, i0, j0, r0, c0);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int q = 0; q < kTile / 8; ++q) {
                const int rr = ty + 8 * q, sr = r0 + rr, sc = c0 + tx;
                if (sr >= 0 && sr < H && sc >= 0 && sc < W) tile[c][rr][tx] = ub[c * HW + (long)sr * W + sc];
            }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kTile / 8; ++q) {
            const int ii = ty + 8 * q, i = i0 + ii, j = j0 + tx;
            if (i < Ho && j < Wo) {
                int tr, tc;
                src_in_block(k, ii, tx, tr, tc);
                const long o = (long)i * Wo + j;
                float pr[C][1], pu[C][1];
                load_softmax<C, 1>(rb + o, HW, pr);
                float mx = tile[0][tr][tc];
#pragma unroll
                for (int c = 0; c < C; ++c) { pu[c][0] = tile[c][tr][tc]; mx = fmaxf(mx, pu[c][0]); }
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) { pu[c][0] = expf(pu[c][0] - mx); s += pu[c][0]; }
#pragma unroll
                for (int c = 0; c < C; ++c) pu[c][0] = pu[c][0] / s;
                if (!BWD) {
#pragma unroll
                    for (int c = 0; c < C; ++c) { const float d = pr[c][0] - pu[c][0]; acc += d * d; }
                } else {
                    float dotr = 0.f, dotu = 0.f;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float d = pr[c][0] - pu[c][0];
                        dotr += pr[c][0] * d;
                        dotu += pu[c][0] * d;
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float d = pr[c][0] - pu[c][0];
                        dr[r_off + b * C * HW + c * HW + o] = a * (pr[c][0] * (d - dotr));
                        tile[c][tr][tc] = -a * (pu[c][0] * (d - dotu));
                    }
                }
            }
        }
        __syncthreads();                                  // the tile is refilled by the next tile (and read back below)
        if (BWD) {
            float* __restrict__ dub = du + u_off + b * C * HW;
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int q = 0; q < kTile / 8; ++q) {
                    const int rr = ty + 8 * q, sr = r0 + rr, sc = c0 + tx;
                    if (sr >= 0 && sr < H && sc >= 0 && sc < W) dub[c * HW + (long)sr * W + sc] = tile[c][rr][tx];
                }
            __syncthreads();
        }
    }
    if (!BWD) {
        const float s = block_sum(acc, red);
        if (threadIdx.x == 0) partials[(long)blockIdx.x * kTerms] = s;
    }
}

// (each returns the grid it launched: the forward's finalize reads one partial row per block)
template <int C> int run_cct_fwd(bool vec, const Heads& h, int D, long HW, long off0, long npix, float* partials, hipStream_t st) {
    const long groups = npix / (vec ? 4 : 1);
    const int grid = grid_for(groups, kMaxBlocks);
    UAPS_LAUNCH_V(vec, cct_fwd_kernel, C, grid, st, h, D, HW, off0, groups, partials);
    return grid;
}
template <int C> int run_cct_bwd(bool vec, const Heads& h, const GradHeads& dh, int D, const float* g, float coef, long HW, long off0, long npix,
                                 hipStream_t st) {
    const long groups = npix / (vec ? 4 : 1);
    UAPS_LAUNCH_V(vec, cct_bwd_kernel, C, grid_for(groups, kMaxBlocks), st, h, dh, D, g, coef, HW, off0, groups);
    return 0;
}
template <int C, bool BWD> int run_rot(int grid, const float* r, const float* u, long r_off, long u_off, int B, int H, int W, int k, int ti, int tj,
                                       const float* g, float coef, float* dr, float* du, float* partials, hipStream_t st) {
    UAPS_LAUNCH_MAIN((rot_cons_kernel<C, BWD>), dim3(grid), dim3(kThreads), 0, st, r, u, r_off, u_off, B, H, W, k, ti, tj, g, coef, dr, du, partials);
    return 0;
}

int cct_fwd_dispatch(int C, bool vec, const Heads& h, int D, long HW, long off0, long npix, float* partials, hipStream_t st) {
#define CALL(K) run_cct_fwd<K>(vec, h, D, HW, off0, npix, partials, st)
    UAPS_BY_C(C, CALL)
#undef CALL
}
int cct_bwd_dispatch(int C, bool vec, const Heads& h, const GradHeads& dh, int D, const float* g, float coef, long HW, long off0, long npix,
                     hipStream_t st) {
#define CALL(K) run_cct_bwd<K>(vec, h, dh, D, g, coef, HW, off0, npix, st)
    UAPS_BY_C(C, CALL)
#undef CALL
}
int rot_dispatch(int C, bool bwd, int grid, const float* r, const float* u, long r_off, long u_off, int B, int H, int W, int k, int ti, int tj,
                 const float* g, float coef, float* dr, float* du, float* partials, hipStream_t st) {
#define CALLF(K) run_rot<K, false>(grid, r, u, r_off, u_off, B, H, W, k, ti, tj, g, coef, dr, du, partials, st)
#define CALLB(K) run_rot<K, true>(grid, r, u, r_off, u_off, B, H, W, k, ti, tj, g, coef, dr, du, partials, st)
    if (bwd) { UAPS_BY_C(C, CALLB) }
    UAPS_BY_C(C, CALLF)
#undef CALLF
#undef CALLB
}

// the window checks every consistency entry point shares: rows [b0, b0 + B) of a batch of C x H x W images
int check_window(int b0, int B, int C, int H, int W) {
    if (b0 < 0 || B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if (C < 2 || C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
    if (4.0 * ((double)b0 + B) * C * H * W >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}
int tiles_of(int H, int W, int k, int& ti, int& tj) {
    const int Ho = (k & 1) ? W : H, Wo = (k & 1) ? H : W;
    ti = (Ho + kTile - 1) / kTile;
    tj = (Wo + kTile - 1) / kTile;
    return ti * tj;
}
}  // namespace

extern "C" int uaps_cct_dct_workspace_bytes(size_t* out) {
    if (!out) return UAPS_EINVAL;
    *out = (size_t)kMaxBlocks * kTerms * sizeof(float);
    return UAPS_OK;
}

extern "C" int uaps_cct_consistency_fwd(const float* const* heads_host, int D, int b0, int B, int C, int H, int W, float* out,
                                        void* workspace, size_t workspace_bytes, uaps_stream_t stream) {
    if (!heads_host || !out || D < 2 || D > UAPS_CCT_MAX_HEADS) return UAPS_EINVAL;
    Heads h{};
    bool vec = ((long)H * W) % 4 == 0;
    for (int k = 0; k < D; ++k) {                     // every argument checked before the first launch
        if (!heads_host[k]) return UAPS_EINVAL;
        h.z[k] = heads_host[k];
        vec = vec && al16(heads_host[k]);
    }
    const int rc = check_window(b0, B, C, H, W);
    if (rc) return rc;
    if (!workspace || workspace_bytes < (size_t)kMaxBlocks * kTerms * sizeof(float)) return UAPS_EWORKSPACE;
    const long HW = (long)H * W, npix = (long)B * HW;
    uaps::account_bytes(4.0 * npix * C * D);
    hipStream_t st = (hipStream_t)stream;
    const int grid = cct_fwd_dispatch(C, vec, h, D, HW, (long)b0 * C * HW, npix, (float*)workspace, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(cct_finalize, dim3(1), dim3(64), 0, st, (const float*)workspace, grid, D, (double)npix * C, out);
    return (int)hipGetLastError();
}

extern "C" int uaps_cct_consistency_bwd(const float* const* heads_host, int D, int b0, int B, int C, int H, int W, const float* grad,
                                        float* const* dheads_host, uaps_stream_t stream) {
    if (!heads_host || !dheads_host || !grad || D < 2 || D > UAPS_CCT_MAX_HEADS) return UAPS_EINVAL;
    Heads h{};
    GradHeads dh{};
    bool vec = ((long)H * W) % 4 == 0;
    for (int k = 0; k < D; ++k) {
        if (!heads_host[k] || !dheads_host[k]) return UAPS_EINVAL;
        h.z[k] = heads_host[k];
        dh.z[k] = dheads_host[k];
        vec = vec && al16(heads_host[k]) && al16(dheads_host[k]);
    }
    const int rc = check_window(b0, B, C, H, W);
    if (rc) return rc;
    const long HW = (long)H * W, npix = (long)B * HW;
    uaps::account_bytes(8.0 * npix * C * D);
    const float coef = (float)(2.0 / ((double)(D - 1) * (double)npix * C));
    cct_bwd_dispatch(C, vec, h, dh, D, grad, coef, HW, (long)b0 * C * HW, npix, (hipStream_t)stream);
    return (int)hipGetLastError();
}

static int rot90_batch_impl(float* amax, const float* x_l, const float* x_u, int B, int Cin, int H, int W, int k, float* out, float* rot_out,
                            uaps_stream_t stream);
extern "C" int uaps_rot90_batch(const float* x_l, const float* x_u, int B, int Cin, int H, int W, int k, float* out, float* rot_out,
                                uaps_stream_t stream) {
    return rot90_batch_impl(uaps::take_hints().out_amax, x_l, x_u, B, Cin, H, W, k, out, rot_out, stream);
}
// (the *_h form: the hints of THIS call as the first argument, nothing thread-local -- see conv_fwd.hip)
extern "C" int uaps_rot90_batch_h(const uaps_call_hints* hints, const float* x_l, const float* x_u, int B, int Cin, int H, int W, int k,
                                  float* out, float* rot_out, uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    return rot90_batch_impl(h.out_amax, x_l, x_u, B, Cin, H, W, k, out, rot_out, stream);
}
static int rot90_batch_impl(float* amax, const float* x_l, const float* x_u, int B, int Cin, int H, int W, int k, float* out, float* rot_out,
                            uaps_stream_t stream) {
    if (!x_l || !x_u || !out || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || k < 0 || k > 3) return UAPS_EINVAL;
    if (!rot_out && (k & 1) && H != W) return UAPS_EINVAL;     // a [B, Cin, W, H] batch cannot share the buffer
    const long n = (long)B * Cin * H * W;
    if (4.0 * 3.0 * (double)n >= kTooBig) return UAPS_ERANGE;
    float* rot = rot_out ? rot_out : out + 2 * n;
    uaps::account_bytes(4.0 * 6.0 * n);                   // x_l, x_u read (x_u twice), 3 n written
    const long n4 = (al16(x_l) && al16(x_u) && al16(out) && n % 4 == 0) ? n / 4 : 0;
    const int cat_blocks = grid_for(n4 > 0 ? 2 * n4 : n, kMaxBlocks);
    int ti, tj;
    const double blocks = (double)cat_blocks + (double)B * Cin * tiles_of(H, W, k, ti, tj);
    if (blocks >= 2147483647.0) return UAPS_ERANGE;
    UAPS_LAUNCH_MAIN(rot90_batch_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, x_l, x_u, out, rot, n, n4, cat_blocks,
                     H, W, k, ti, tj, amax);
    return (int)hipGetLastError();
}

extern "C" int uaps_rot_consistency_fwd(const float* r, int r_b0, const float* u, int u_b0, int B, int C, int H, int W, int k, float* out2,
                                        void* workspace, size_t workspace_bytes, uaps_stream_t stream) {
    if (!r || !u || !out2 || k < 0 || k > 3) return UAPS_EINVAL;
    int rc = check_window(r_b0, B, C, H, W);
    if (!rc) rc = check_window(u_b0, B, C, H, W);
    if (rc) return rc;
    if (!workspace || workspace_bytes < (size_t)kMaxBlocks * kTerms * sizeof(float)) return UAPS_EWORKSPACE;
    const long HW = (long)H * W, npix = (long)B * HW;
    int ti, tj;
    const long tiles = (long)B * tiles_of(H, W, k, ti, tj);
    const int grid = (int)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
    uaps::account_bytes(8.0 * npix * C);
    hipStream_t st = (hipStream_t)stream;
    rot_dispatch(C, false, grid, r, u, (long)r_b0 * C * HW, (long)u_b0 * C * HW, B, H, W, k, ti, tj, nullptr, 0.f, nullptr, nullptr,
                 (float*)workspace, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(cct_finalize, dim3(1), dim3(64), 0, st, (const float*)workspace, grid, 2, (double)npix * C, out2);
    return (int)hipGetLastError();
}

extern "C" int uaps_rot_consistency_bwd(const float* r, int r_b0, const float* u, int u_b0, int B, int C, int H, int W, int k, const float* grad,
                                        float* dr, float* du, uaps_stream_t stream) {
    if (!r || !u || !grad || !dr || !du || k < 0 || k > 3) return UAPS_EINVAL;
    int rc = check_window(r_b0, B, C, H, W);
    if (!rc) rc = check_window(u_b0, B, C, H, W);
    if (rc) return rc;
    const long HW = (long)H * W, npix = (long)B * HW;
    int ti, tj;
    const long tiles = (long)B * tiles_of(H, W, k, ti, tj);
    const int grid = (int)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
    uaps::account_bytes(16.0 * npix * C);
    rot_dispatch(C, true, grid, r, u, (long)r_b0 * C * HW, (long)u_b0 * C * HW, B, H, W, k, ti, tj, grad, (float)(2.0 / ((double)npix * C)),
                 dr, du, nullptr, (hipStream_t)stream);
    return (int)hipGetLastError();
}
