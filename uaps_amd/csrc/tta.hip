// Multi-scale + horizontal-flip test-time augmentation for gfx950 (include/uaps_hip.h, uaps_tta_views / uaps_tta_fold): the reference's
// BaseNet.forward(x, tta=True) (utilities/base.py:24-46) sums, over the scales and over {plain, flipped}, the softmax of a forward of
// the resized batch, resized back to the input's size.  Two kernels stand around the network's forwards:
//   tta_views_kernel   the input side of ONE scale: x [B,Cin,H,W] -> [2B,Cin,h,w], the bilinear resize (align_corners=True) and,
//                      behind it, the same values stored mirrored (images B..2B-1), so that one forward of 2B images serves both views
//   tta_fold_kernel    the output side of ALL scales: a lane owns V consecutive output pixels and keeps their C running sums in
//                      registers; per scale, plain then flipped, it takes the softmax of the logits at the four source corners, mixes
//                      them bilinearly and adds -- ((((p0 + f0) + p1) + f1) + ...), the reference's order -- and at the end writes the
//                      sum, its arg-max and the confidence.  No atomics, no cross-lane sums: two runs give the same bits.
// The bilinear arithmetic is torch's fp32 align_corners=True form: r = (in - 1) / (out - 1) as a float (0 when out == 1, formed on the
// host), src = r * dst, i0 = (int) src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1,
// value = l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11).  src is rounded on its own (mul_rn): fused into l1 it would
// be a different weight.  A flipped forward is un-flipped BEFORE its resize: the output column whose neighbours are x0, x1 reads the
// columns w - 1 - x0 and w - 1 - x1 of image B + b.
#include "loss_common.hpp"               // uaps::pixel (the softmax of a pixel's logits), UAPS_BY_C, UAPS_LAUNCH_V
#include "rn_math.hpp"

namespace {
using uaps::kThreads; using uaps::kTooBig; using uaps::grid_for; using uaps::al16;
constexpr int kMaxScales = UAPS_TTA_MAX_SCALES;
constexpr int kMaxBlocks = 1 << 20;      // every tensor is below 2 GiB: a grid never needs more; the lanes stride over the rest anyway

// source index pair and the weight of the second: torch's align_corners=True map of destination index d
__device__ __forceinline__ void corners(float r, int d, int in, int& i0, int& i1, float& l1) {
    const float src = uaps::mul_rn(r, (float)d);
    i0 = min((int)src, in - 1);          // src <= in - 1 up to its rounding: the clamp never moves a valid index
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
}

struct ViewsArgs {
    int B, Cin, H, W, h, w, flip;
    float rh, rw;
    const float* x; float* out;
};

// one lane per element of the resized batch; the flipped copy is the same value at the mirrored column of image B + b
__global__ __launch_bounds__(kThreads) void tta_views_kernel(ViewsArgs a) {
    const long plane = (long)a.h * a.w, per = (long)a.Cin * plane, n = (long)a.B * per;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        const long bc = i / plane, pix = i - bc * plane;
        const int y = (int)(pix / a.w), j = (int)(pix - (long)y * a.w);
        int y0, y1, x0, x1; float ly, lx;
        corners(a.rh, y, a.H, y0, y1, ly);
        corners(a.rw, j, a.W, x0, x1, lx);
        const float* p = a.x + bc * (long)a.H * a.W;
        const float v00 = p[(long)y0 * a.W + x0], v01 = p[(long)y0 * a.W + x1];
        const float v10 = p[(long)y1 * a.W + x0], v11 = p[(long)y1 * a.W + x1];
        const float my = 1.f - ly, mx = 1.f - lx;
        const float v = my * (mx * v00 + lx * v01) + ly * (mx * v10 + lx * v11);
        a.out[i] = v;
        if (a.flip) a.out[n + bc * plane + (long)y * a.w + (a.w - 1 - j)] = v;
    }
}

struct FoldArgs {
    int S, B, H, W, flip;
    const float* z[kMaxScales];
    int h[kMaxScales], w[kMaxScales];
    float rh[kMaxScales], rw[kMaxScales];
    float* probs; long long* mask; float* conf;
};

// q = softmax of the C logits at p (class stride hw)
template <int C>
__device__ __forceinline__ void corner_softmax(const float* __restrict__ p, long hw, float (&q)[C]) {
    float z[C][1], mx[1], lse[1];
    uaps::pixel::load_logits<C, 1>(p, hw, z);
    uaps::pixel::softmax_inplace<C, 1>(z, mx, lse);
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = z[c][0];
}

// the bilinear mix of the softmax at the four corners (rows y0, y1; columns x0, x1) of one image's logits
template <int C>
__device__ __forceinline__ void mixed_softmax(const float* __restrict__ img, int w, long hw, int y0, int y1, int x0, int x1, float ly,
                                              float lx, float (&out)[C]) {
    float q00[C], q01[C], q10[C], q11[C];
    corner_softmax<C>(img + (long)y0 * w + x0, hw, q00);
    corner_softmax<C>(img + (long)y0 * w + x1, hw, q01);
    corner_softmax<C>(img + (long)y1 * w + x0, hw, q10);
    corner_softmax<C>(img + (long)y1 * w + x1, hw, q11);
    const float my = 1.f - ly, mx = 1.f - lx;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = my * (mx * q00[c] + lx * q01[c]) + ly * (mx * q10[c] + lx * q11[c]);
}

// V = 4 needs W % 4 == 0 (a group never straddles two rows) and 16-byte aligned outputs
template <int C, int V>
__global__ __launch_bounds__(kThreads) void tta_fold_kernel(FoldArgs a) {
    const long HW = (long)a.H * a.W, groups = (long)a.B * HW / V;
    const float views = (float)(a.S * (a.flip ? 2 : 1));
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long)gridDim.x * kThreads) {
        const long n = g * V;
        const int b = (int)(n / HW);
        const long pix = n - (long)b * HW;
        const int y = (int)(pix / a.W), x = (int)(pix - (long)y * a.W);
        float acc[C][V];
        for (int s = 0; s < a.S; ++s) {
            const int hs = a.h[s], ws = a.w[s];
            const long hw = (long)hs * ws;
            const float* plain = a.z[s] + (long)b * C * hw;
            const float* flipped = a.z[s] + ((long)a.B + b) * C * hw;
            int y0, y1; float ly;
            corners(a.rh[s], y, hs, y0, y1, ly);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                int x0, x1; float lx;
                corners(a.rw[s], x + v, ws, x0, x1, lx);
                float t[C];
                mixed_softmax<C>(plain, ws, hw, y0, y1, x0, x1, ly, lx, t);
                if (s == 0) {
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c][v] = t[c];
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c][v] += t[c];
                }
                if (a.flip) {
                    mixed_softmax<C>(flipped, ws, hw, y0, y1, ws - 1 - x0, ws - 1 - x1, ly, lx, t);
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c][v] += t[c];
                }
            }
        }
        if (a.probs) uaps::pixel::store_planes<C, V>(a.probs + (long)b * C * HW + pix, HW, acc);
        if (a.mask || a.conf) {
            int am[V];
            uaps::pixel::argmax_logits<C, V>(acc, am);
            if (a.mask) {
                if constexpr (V == 4) {
                    longlong2* m = reinterpret_cast<longlong2*>(a.mask + n);
                    m[0] = make_longlong2(am[0], am[1]);
                    m[1] = make_longlong2(am[2], am[3]);
                } else {
                    a.mask[n] = am[0];
                }
            }
            if (a.conf) {
                float cf[1][V];
#pragma unroll
                for (int v = 0; v < V; ++v) cf[0][v] = uaps::pixel::pick<C, V>(acc, v, am[v]) / views;
                uaps::pixel::store_planes<1, V>(a.conf + n, 0, cf);
            }
        }
    }
}

inline float ratio(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }
inline bool too_big(double elems, double bytes_each) { return elems * bytes_each >= kTooBig; }

template <int C>
int launch_fold(const FoldArgs& a, bool vec, hipStream_t st) {
    const long groups = (long)a.B * a.H * a.W / (vec ? 4 : 1);
    const int grid = grid_for(groups, kMaxBlocks);
    UAPS_LAUNCH_V(vec, tta_fold_kernel, C, grid, st, a);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int uaps_tta_views(const uaps_tta_views_call* call) {
    uaps_tta_views_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.x || !c.out || (c.flip != 0 && c.flip != 1)) return UAPS_EINVAL;
    if (c.B <= 0 || c.Cin <= 0 || c.H <= 0 || c.W <= 0 || c.h <= 0 || c.w <= 0) return UAPS_EINVAL;
    const double planes = (double)c.B * c.Cin;
    if (too_big(planes * c.H * c.W, 4.0) || too_big(planes * (c.flip ? 2 : 1) * c.h * c.w, 4.0)) return UAPS_ERANGE;
    ViewsArgs a;
    a.B = c.B; a.Cin = c.Cin; a.H = c.H; a.W = c.W; a.h = c.h; a.w = c.w; a.flip = c.flip;
    a.rh = ratio(c.H, c.h); a.rw = ratio(c.W, c.w);
    a.x = c.x; a.out = c.out;
    const long n = (long)c.B * c.Cin * c.h * c.w;
    uaps::account_bytes(4.0 * (planes * c.H * c.W + (c.flip ? 2.0 : 1.0) * (double)n));
    UAPS_LAUNCH_MAIN(tta_views_kernel, dim3(grid_for(n, kMaxBlocks)), dim3(kThreads), 0, (hipStream_t)c.stream, a);
    return (int)hipGetLastError();
}

extern "C" int uaps_tta_fold(const uaps_tta_fold_call* call) {
    uaps_tta_fold_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if ((!c.probs_sum && !c.mask && !c.conf) || (c.flip != 0 && c.flip != 1)) return UAPS_EINVAL;
    if (c.B <= 0 || c.C <= 0 || c.H <= 0 || c.W <= 0) return UAPS_EINVAL;
    if (c.C < 2 || c.C > UAPS_MAX_CLASSES || c.S < 1 || c.S > kMaxScales) return UAPS_ERANGE;
    const double images = (double)c.B * (c.flip ? 2 : 1), pixels = (double)c.B * c.H * c.W;
    double read = 0.0;
    for (int s = 0; s < c.S; ++s) {
        if (!c.logits[s] || c.h[s] <= 0 || c.w[s] <= 0) return UAPS_EINVAL;
        const double elems = images * c.C * c.h[s] * c.w[s];
        if (too_big(elems, 4.0)) return UAPS_ERANGE;
        read += 4.0 * elems;
    }
    // the outputs the call writes: a NULL one is no tensor
    if ((c.probs_sum && too_big(pixels * c.C, 4.0)) || (c.mask && too_big(pixels, 8.0)) || (c.conf && too_big(pixels, 4.0))) return UAPS_ERANGE;
    FoldArgs a;
    memset(&a, 0, sizeof a);
    a.S = c.S; a.B = c.B; a.H = c.H; a.W = c.W; a.flip = c.flip;
    for (int s = 0; s < c.S; ++s) {
        a.z[s] = c.logits[s]; a.h[s] = c.h[s]; a.w[s] = c.w[s];
        a.rh[s] = ratio(c.h[s], c.H); a.rw[s] = ratio(c.w[s], c.W);
    }
    a.probs = c.probs_sum; a.mask = (long long*)c.mask; a.conf = c.conf;
    const bool vec = c.W % 4 == 0 && al16(c.probs_sum) && al16(c.mask) && al16(c.conf);
    uaps::account_bytes(read + pixels * ((c.probs_sum ? 4.0 * c.C : 0.0) + (c.mask ? 8.0 : 0.0) + (c.conf ? 4.0 : 0.0)));
    hipStream_t st = (hipStream_t)c.stream;
#define UAPS_TTA_FOLD(Cc) launch_fold<Cc>(a, vec, st)
    UAPS_BY_C(c.C, UAPS_TTA_FOLD);
#undef UAPS_TTA_FOLD
}
