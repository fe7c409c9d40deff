// What the gradient fan-in kernels share (perturb.hip: fanin_perturbed_kernel; enc_glue.hip: the form that also sums for the
// BatchNorm backward): the flat-index arithmetic, the kernel argument record and the entry points' argument checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uaps_hip.h"

namespace uaps {
inline bool fan_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// e = q * d + r for the flat element index of the fan kernels: a shift when d is a power of two (`sh` = log2 d, every level of the
// 256 x 256 / 512 x 512 configurations), one 32-bit division when both fit (the 640 x 640 ResNet maps), the 64-bit division otherwise.
// The 64-bit form alone cost the fan kernels a fifth of their time: they are VALU-co-limited by the two Philox calls per element.
__device__ __forceinline__ void fan_divmod(long e, long d, int sh, long& q, long& r) {
    if (sh >= 0) { q = e >> sh; r = e & (d - 1); }
    else if (((unsigned long)e | (unsigned long)d) >> 32 == 0) { const uint32_t q32 = (uint32_t)e / (uint32_t)d; q = q32; r = (uint32_t)e - q32 * (uint32_t)d; }
    else { q = e / d; r = e - q * d; }
}
inline int fan_log2(long d) { return d > 0 && (d & (d - 1)) == 0 ? __builtin_ctzl((unsigned long)d) : -1; }
constexpr int kFanMax = 8, kFanGroups = 4;
static_assert(kFanGroups == 4, "the fan kernels derive the statistics group of an image by three comparisons");
struct FanInArgs {
    const float4* g[kFanMax];
    const uchar4* keep[kFanMax];
    uint64_t off[kFanMax][kFanGroups];
    int mode[kFanMax];
    uint64_t seed;
    float range, p, scale;
    int n, B, Bg;
    long chw4, hw4;
    int W;
    int sh_chw4, sh_hw4, sh_w;      // log2 of chw4 / hw4 / W, or -1 (fan_divmod)
    int Ho;                         // H / 2 (mode 4)
    const uint32_t* st;             // step state (philox.hpp) or NULL
};
// validates the arguments of uaps_fanin_perturbed and fills the kernel's record
inline int fanin_args(const float* const* g, const int* mode, const uint8_t* const* keep, const uint64_t* offsets, int n, int groups,
                      uint64_t seed, float range, float p, int B, int C, int H, int W, const float* out, FanInArgs& a) {
    if (!g || !mode || !out || n < 1 || n > kFanMax || groups < 1 || groups > kFanGroups || B <= 0 || C <= 0 || H <= 0 || W <= 0 ||
        B % groups)
        return UAPS_EINVAL;
    const long HW = (long)H * W;
    if (HW % 4 || !fan_al16(out)) return UAPS_EINVAL;
    for (int k = 0; k < n; ++k) {
        if (!g[k] || !fan_al16(g[k]) || mode[k] < 0 || mode[k] > 4) return UAPS_EINVAL;
        if ((mode[k] == 3 || mode[k] == 4) && (!keep || !keep[k] || (reinterpret_cast<uintptr_t>(keep[k]) & 3))) return UAPS_EINVAL;
        if (mode[k] == 4 && (H % 2 || W % 4)) return UAPS_EINVAL;
        if ((mode[k] == 1 || mode[k] == 2) && !offsets) return UAPS_EINVAL;
        a.g[k] = (const float4*)g[k]; a.mode[k] = mode[k]; a.keep[k] = keep ? (const uchar4*)keep[k] : nullptr;
        for (int q = 0; q < groups; ++q) a.off[k][q] = offsets ? offsets[(size_t)k * groups + q] : 0;
    }
    a.seed = seed; a.range = range; a.p = p; a.scale = 1.f / (1.f - p); a.n = n; a.B = B; a.Bg = B / groups;
    a.st = (const uint32_t*)uaps_get_step_state();
    a.chw4 = (long)C * HW / 4; a.hw4 = HW / 4; a.W = W; a.Ho = H / 2;
    a.sh_chw4 = fan_log2(a.chw4); a.sh_hw4 = fan_log2(a.hw4); a.sh_w = fan_log2(W);
    return UAPS_OK;
}
// every incoming gradient once (mode 4: the pooled gradient and its index bytes), the keep masks, the sum once
inline double fanin_bytes(const int* mode, int n, int B, int C, long HW) {
    double by = 4.0 * B * C * HW;
    for (int k = 0; k < n; ++k) by += mode[k] == 4 ? 5.0 * B * C * HW / 4 : 4.0 * B * C * HW + (mode[k] == 3 ? (double)B * HW : 0.0);
    return by;
}
}  // namespace uaps
