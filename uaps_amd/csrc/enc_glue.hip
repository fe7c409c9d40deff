// The encoder's glue launches folded into their neighbours, for gfx950:
//   enc_fanin_bn_sums_kernel   the feature fan-in (perturb.hip) that also forms the backward sums of the BatchNorm that wrote the feature
//   enc_bn_apply_pool_kernel   the BatchNorm apply pass (norm_act.hip) that also writes the 2x2 max-pool of the next encoder level
// Both repeat the arithmetic of the launches they replace expression for expression: every result is those launches' bits
// (tests/test_gpu_enc_glue.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uaps_hip.h"
#include "rn_math.hpp"
#include "philox.hpp"
#include "hints.hpp"
#include "bn_pieces.hpp"
#include "fan_pieces.hpp"
using uaps::mul_rn; using uaps::add_rn; using uaps::U4; using uaps::philox4x32_10; using uaps::u01;
using uaps::fan_divmod; using uaps::kFanMax; using uaps::kFanGroups; using uaps::FanInArgs; using uaps::fanin_args; using uaps::fanin_bytes;
using uaps::fan_al16;

namespace {
constexpr int kThreads = uaps::kBnThreads;
constexpr int kChunk = uaps::kBnChunk;

// ---- the same fan-in, also forming the backward sums of the BatchNorm that produced the feature map ------------------
// The summed gradient is d(activation) of that BatchNorm + LeakyReLU; bn_bwd_sums_kernel<true, false> (norm_act.hip) would read it
// back, with the raw conv output y, for nothing but two sums per chunk.  Here the block geometry is that kernel's -- grid (chunks of
// 4096 floats, planes), thread t owns the float4 at lo + 4 t + 1024 j -- and each thread runs that kernel's arithmetic on the float4 it
// just summed (the same element order per thread, the same block_sum2), so the partials [(c B + b) nch + chunk] are its bits.  Per
// element the gradient is fanin_perturbed_kernel's: the same modes, Philox counters (the flat float4 index e) and summation order.
struct FanBnArgs {
    const float* y; const float* mean; const float* invstd; const float* gamma; const float* beta;
    float2* partials;
    float slope;
    int C, nch;
    long HW;
};
__global__ __launch_bounds__(kThreads) void enc_fanin_bn_sums_kernel(FanInArgs a, float4* __restrict__ out, FanBnArgs s) {
    const uint64_t seed = uaps::step_key(a.seed, a.st);
    const int plane = blockIdx.y, chunk = blockIdx.x;
    const int ib = plane / s.C, c = plane - ib * s.C;
    const int grp = (ib >= a.Bg) + (ib >= 2 * a.Bg) + (ib >= 3 * a.Bg);      // b / Bg for <= kFanGroups = 4 groups
    const float mu = s.mean[grp * s.C + c], is = s.invstd[grp * s.C + c], sc = s.gamma[c] * is, sh = s.beta[c];
    const long b = ib, pbase = (long)plane * s.HW;
    const long lo = (long)chunk * uaps::kBnChunk, hi = min(s.HW, lo + (long)uaps::kBnChunk);
    float s1 = 0.f, s2 = 0.f;
    for (long i = lo + 4 * threadIdx.x; i < hi; i += 4 * kThreads) {
        const long e = (pbase + i) >> 2, pix = i >> 2, ce = (long)c * a.hw4 + pix;      // float4 index: flat, in the plane, in the image
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < kFanMax; ++k) {
            if (k >= a.n) break;
            float4 v;
            if (a.mode[k] == 4) {               // 4 consecutive pixels of row h <- 2 pooled pixels of row h/2
                long hh, ww;
                fan_divmod(i, a.W, a.sh_w, hh, ww);
                const int h = (int)hh, w = (int)ww, Wo = a.W / 2;
                const long po = ((long)plane * a.Ho + h / 2) * (long)Wo + w / 2;
                const float2 gp = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(a.g[k]) + po);
                const uchar2 ix = *reinterpret_cast<const uchar2*>(reinterpret_cast<const uint8_t*>(a.keep[k]) + po);
                const int base = (h & 1) * 2;
                v.x = ix.x == base ? gp.x : 0.f; v.y = ix.x == base + 1 ? gp.x : 0.f;
                v.z = ix.y == base ? gp.y : 0.f; v.w = ix.y == base + 1 ? gp.y : 0.f;
            } else {
                v = a.g[k][e];
            }
            if (a.mode[k] == 1) {
                const U4 r = philox4x32_10(a.off[k][grp] + (uint64_t)ce, seed);
                const float n0 = (2.f * u01(r.x) - 1.f) * a.range, n1 = (2.f * u01(r.y) - 1.f) * a.range;
                const float n2 = (2.f * u01(r.z) - 1.f) * a.range, n3 = (2.f * u01(r.w) - 1.f) * a.range;
                v.x = add_rn(mul_rn(v.x, n0), v.x); v.y = add_rn(mul_rn(v.y, n1), v.y);
                v.z = add_rn(mul_rn(v.z, n2), v.z); v.w = add_rn(mul_rn(v.w, n3), v.w);
            } else if (a.mode[k] == 2) {
                const U4 r = philox4x32_10(a.off[k][0] + (uint64_t)e, seed);
                v.x = u01(r.x) >= a.p ? v.x * a.scale : 0.f; v.y = u01(r.y) >= a.p ? v.y * a.scale : 0.f;
                v.z = u01(r.z) >= a.p ? v.z * a.scale : 0.f; v.w = u01(r.w) >= a.p ? v.w * a.scale : 0.f;
            } else if (a.mode[k] == 3) {
                const uchar4 m = a.keep[k][b * a.hw4 + pix];
                v.x = m.x ? v.x : 0.f; v.y = m.y ? v.y : 0.f; v.z = m.z ? v.z : 0.f; v.w = m.w ? v.w : 0.f;
            }
            if (k == 0) acc = v;
            else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
        }
        out[e] = acc;
        const float4 y4 = *reinterpret_cast<const float4*>(s.y + pbase + i);
        const float g[4] = {acc.x, acc.y, acc.z, acc.w};
        const float yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = uaps::dpre(g[k], yy[k], mu, sc, sh, s.slope);
            s1 += d; s2 += d * ((yy[k] - mu) * is);
        }
    }
    const float2 r = uaps::block_sum2(s1, s2);
    if (threadIdx.x == 0) s.partials[((long)c * (gridDim.y / s.C) + ib) * s.nch + chunk] = r;
}

// ---- forward pass 2 of an encoder block's last BatchNorm: the activated tensor AND the 2x2 max-pool of the next level ------
// bn_apply_kernel<true, false> of norm_act.hip (no residual) whose thread owns 8 columns of two adjacent rows instead of 16 consecutive floats: the four
// pooled values and arg-max bytes of that patch leave from registers, with maxpool2x2_fwd_kernel's scan (perturb.hip: first maximum
// in scan order wins, a NaN replaces whatever came before it), so that launch and its re-read of the activated tensor go away.
// Needs W = 2^w8sh * 8 dividing kChunk / 2 (a chunk is whole row pairs; 256 threads x (2 x 8) floats = one chunk) and H even.
__global__ __launch_bounds__(kThreads) void enc_bn_apply_pool_kernel(const float* __restrict__ y, float* __restrict__ out, float* __restrict__ pooled,
                                                                 uint8_t* __restrict__ idx, int C, long HW, int W, int w8sh,
                                                                 const float* __restrict__ mean, const float* __restrict__ coef, float slope,
                                                                 int Bg, float* __restrict__ amax) {
    const int plane = blockIdx.y, chunk = blockIdx.x;
    const int b = plane / C, c = plane - b * C, g = b / Bg;
    const float* cf = coef + (long)g * 4 * C;
    const float mu = mean[g * C + c], sc = cf[c], sh = cf[C + c];
    const long pbase = (long)plane * HW;
    const long lo = (long)chunk * kChunk, hi = min(HW, lo + (long)kChunk);
    const int r = threadIdx.x >> w8sh, cg = threadIdx.x - (r << w8sh);      // row pair of the chunk, group of 8 columns
    const long i = lo + (long)r * 2 * W + cg * 8;
    float m = 0.f;
    if (i < hi) {                                        // (hi - lo is a multiple of 2 W: the whole patch is inside)
        const float* p = y + pbase + i;
        const float4 a0 = *reinterpret_cast<const float4*>(p), a1 = *reinterpret_cast<const float4*>(p + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(p + W), b1 = *reinterpret_cast<const float4*>(p + W + 4);
        const float v[2][8] = {{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w}};
        float z[2][8];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                z[q][k] = (v[q][k] - mu) * sc + sh;
                z[q][k] = z[q][k] > 0.f ? z[q][k] : z[q][k] * slope;
                m = fmaxf(m, fabsf(z[q][k]));
            }
        float* o = out + pbase + i;
        *reinterpret_cast<float4*>(o) = make_float4(z[0][0], z[0][1], z[0][2], z[0][3]);
        *reinterpret_cast<float4*>(o + 4) = make_float4(z[0][4], z[0][5], z[0][6], z[0][7]);
        *reinterpret_cast<float4*>(o + W) = make_float4(z[1][0], z[1][1], z[1][2], z[1][3]);
        *reinterpret_cast<float4*>(o + W + 4) = make_float4(z[1][4], z[1][5], z[1][6], z[1][7]);
        float pv[4]; uint8_t ix[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float mx = z[0][2 * k]; int w = 0;
            if (z[0][2 * k + 1] > mx || z[0][2 * k + 1] != z[0][2 * k + 1]) { mx = z[0][2 * k + 1]; w = 1; }
            if (z[1][2 * k] > mx || z[1][2 * k] != z[1][2 * k]) { mx = z[1][2 * k]; w = 2; }
            if (z[1][2 * k + 1] > mx || z[1][2 * k + 1] != z[1][2 * k + 1]) { mx = z[1][2 * k + 1]; w = 3; }
            pv[k] = mx; ix[k] = (uint8_t)w;
        }
        const long oo = (pbase + i - (long)cg * 8) / 4 + cg * 4;      // (plane, row pair) start of the pooled map + 4 columns per group
        *reinterpret_cast<float4*>(pooled + oo) = make_float4(pv[0], pv[1], pv[2], pv[3]);
        *reinterpret_cast<uchar4*>(idx + oo) = make_uchar4(ix[0], ix[1], ix[2], ix[3]);
    }
    if (amax != nullptr) {                               // uniform branch
        __shared__ float sm[16];
        uaps::block_amax_to(amax, m, sm);
    }
}
}  // namespace

// uaps_fanin_perturbed for a feature map that a train-mode BatchNorm + LeakyReLU (no dropout) produced from y: the same `out`, and in
// the same pass the backward sums of that BatchNorm over (out, y) -- partials float2 [C][B][ceil(H W / 4096)], the bits the sums pass
// of uaps_bn_act_bwd_grouped would form; uaps_bn_act_bwd_partials_h then runs the dx pass alone.  Whatever uaps_fanin_perturbed
// refuses is refused alike; misaligned y / partials or more than 65535 planes: UAPS_ENOFORM, nothing launched, nothing written.
extern "C" int uaps_fanin_perturbed_bn_sums_h(const uaps_call_hints* hints, const float* const* g, const int* mode, const uint8_t* const* keep,
                                              const uint64_t* offsets, int n, int groups, uint64_t seed, float range, float p, int B, int C,
                                              int H, int W, float* out, const float* y, const float* gamma, const float* beta,
                                              const float* save_mean, const float* save_invstd, float slope, void* partials,
                                              uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    (void)h;
    if (!y || !gamma || !beta || !save_mean || !save_invstd || !partials) return UAPS_EINVAL;
    if (g && mode && n >= 1 && n <= kFanMax)
        for (int k = 0; k < n; ++k) if (g[k] && !fan_al16(g[k])) return UAPS_ENOFORM;
    if (!fan_al16(out) || !fan_al16(y) || (reinterpret_cast<uintptr_t>(partials) & 7) || ((long)H * W) % 4) return UAPS_ENOFORM;
    if ((long)B * C > 65535) return UAPS_ENOFORM;      // planes ride on gridDim.y
    FanInArgs a{};
    const int rc = fanin_args(g, mode, keep, offsets, n, groups, seed, range, p, B, C, H, W, out, a);
    if (rc) return rc;
    const long HW = (long)H * W;
    FanBnArgs s{};
    s.y = y; s.mean = save_mean; s.invstd = save_invstd; s.gamma = gamma; s.beta = beta; s.partials = (float2*)partials;
    s.slope = slope; s.C = C; s.HW = HW; s.nch = (int)((HW + uaps::kBnChunk - 1) / uaps::kBnChunk);
    uaps::account_bytes(fanin_bytes(mode, n, B, C, HW) + 4.0 * B * C * HW);      // + y once
    hipLaunchKernelGGL(enc_fanin_bn_sums_kernel, dim3(s.nch, B * C), dim3(kThreads), 0, (hipStream_t)stream, a, (float4*)out, s);
    return (int)hipGetLastError();
}


// H even, W a multiple of 8 (a thread pools a 2 x 8 patch) and 2 W dividing the 4096-float chunk (a chunk is whole row pairs)
extern "C" int uaps_bn_apply_pool_support(int H, int W) {
    if (H < 2 || W < 8 || H % 2 || W % 8 || uaps::kBnChunk % (2 * W)) return UAPS_ENOFORM;
    return UAPS_OK;
}

// the apply pass of bn_fwd_train_impl (norm_act.hip) in that form; the caller has checked the form and the pointers
void uaps::launch_bn_apply_pool(const float* y, float* out, float* pooled, uint8_t* idx, int B, int C, int H, int W, const float* mean,
                                const float* coef, float slope, int Bg, float* amax, hipStream_t stream) {
    const long HW = (long)H * W;
    hipLaunchKernelGGL(enc_bn_apply_pool_kernel, dim3((unsigned)((HW + kChunk - 1) / kChunk), B * C), dim3(kThreads), 0, stream, y, out, pooled, idx, C,
                       HW, W, __builtin_ctz((unsigned)W / 8), mean, coef, slope, Bg, amax);
}
