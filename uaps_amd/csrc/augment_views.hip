// On-device input pipeline for gfx950, any recipe, one or two views per source (include/uaps_hip.h, uaps_augment_views):
// the dataset variants of the reference's loaders -- DAGM / KoSDD2 / MTiles UAPS_dataloaders.py, UCC/UCC_dataloaders.py:149-168
// (weak and strong views of one unlabelled image) -- run the stages of utilities/dataloaders.py in other orders, on 1 or 3
// channels, and add GridDistortion, ColorJitter and PixelDropout.  csrc/augment.hip stays the NEU path; this file is ONE gather
// kernel that interprets a small per-(view, image) program (uaps_view_row): a thread owns one output pixel of one view.
//
// Geometry (resize-nearest, flips, quarter turns) is a coordinate map applied first; the program then runs in that working frame.
// GRID (bilinear resample along two 1-D maps) and BLUR (box window) split the program into three segments:
//   level0  source pixel -> ops in front of GRID         evaluated at the four bilinear corners
//   level1  GRID sample  -> ops between GRID and BLUR     evaluated at every blur tap
//   level2  BLUR mean    -> ops behind BLUR               evaluated once
// level2(y, x, n) is "the value of the image at working-frame pixel (y, x) after the first n ops"; the main kernel calls it with
// the whole program, the CONTRAST pre-pass with the prefix in front of that op.
// PARITY UNPINNED: cv2 and albumentations are not in the build image; the arithmetic is the one include/uaps_hip.h writes down
// (tests/augment_views_ref.py restates it stage by stage in numpy), not a measured equality with either library.
#include "call_common.hpp"
#include "philox.hpp"

namespace {
using uaps::U4; using uaps::philox4x32_10; using uaps::u01; using uaps::pick;
constexpr int kThreads = 256;
constexpr int kMaxOps = UAPS_AUG_MAX_OPS;

// cv2 BORDER_REFLECT_101; callers pass i in [-n, 2n), so the loop of csrc/augment.hip runs at most a few times
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}
__device__ __forceinline__ float clip255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// the kernels' arguments: the call without its host-only fields
struct Args {
    int V, B, Hs, Ws, Cs, Ho, Wo;
    const uint8_t* images; const uint8_t* masks; const uaps_view_row* rows;
    const float* grid_ys; const float* grid_xs; const float* noise; const float* drop_u;
    uint64_t seed;
    float mean[3], stdv[3];
    float* out; int64_t* out_mask;
    float* m;                    // [V * B] contrast means (workspace), null when no program holds CONTRAST
    uint32_t* partial;           // [V * B][blocks per frame] (workspace)
};

// one (view, image): uniform over a wavefront
struct View {
    const uint8_t* src; const uaps_view_row* row; const float* noise; const float* drop; const float* gys; const float* gxs;
    int Hs, Ws, Cs, Ho, Wo, hflip, vflip, rot;
    int nops, g, k, c, r;        // program length; index of GRID / BLUR / CONTRAST (-1: none); blur radius
    float m;
    uint64_t seed, ctr;          // Philox key and the counter of pixel (0, 0) of this (view, image)
};

__device__ __forceinline__ View make_view(const Args& a, int v, int b) {
    View w;
    const long vb = (long)v * a.B + b, per = (long)a.Ho * a.Wo;
    w.src = a.images + (long)b * a.Hs * a.Ws * a.Cs;
    w.row = a.rows + vb;
    w.noise = a.noise ? a.noise + vb * a.Cs * per : nullptr;
    w.drop = a.drop_u ? a.drop_u + vb * per : nullptr;
    w.gys = a.grid_ys ? a.grid_ys + vb * a.Ho : nullptr;
    w.gxs = a.grid_xs ? a.grid_xs + vb * a.Wo : nullptr;
    w.Hs = a.Hs; w.Ws = a.Ws; w.Cs = a.Cs; w.Ho = a.Ho; w.Wo = a.Wo;
    w.hflip = w.row->hflip; w.vflip = w.row->vflip; w.rot = w.row->rot_k & 3;
    w.nops = kMaxOps; w.g = w.k = w.c = -1; w.r = 0;
    for (int i = kMaxOps - 1; i >= 0; --i) {
        const int op = w.row->op[i];
        if (op == UAPS_AUG_END) w.nops = i;
    }
    for (int i = 0; i < w.nops; ++i) {
        const int op = w.row->op[i];
        if (op == UAPS_AUG_GRID && w.gys && w.gxs) w.g = i;
        if (op == UAPS_AUG_BLUR) { w.k = i; w.r = min(max((int)w.row->a[i], 1), 7) / 2; }
        if (op == UAPS_AUG_CONTRAST) w.c = i;
    }
    w.m = 0.f;
    w.seed = a.seed; w.ctr = (uint64_t)(vb * per);
    return w;
}

// working-frame pixel (y, x) -> the source pixel: np.rot90 undone, flips undone, INTER_NEAREST (csrc/augment.hip's map)
__device__ __forceinline__ void source_of(const View& w, int y, int x, int& sy, int& sx) {
    int ry, rx;
    if (w.rot == 0) { ry = y; rx = x; }
    else if (w.rot == 1) { ry = x; rx = w.Wo - 1 - y; }
    else if (w.rot == 2) { ry = w.Ho - 1 - y; rx = w.Wo - 1 - x; }
    else { ry = w.Ho - 1 - x; rx = y; }
    if (w.vflip) ry = w.Ho - 1 - ry;
    if (w.hflip) rx = w.Wo - 1 - rx;
    sy = min((int)(((long)ry * w.Hs) / w.Ho), w.Hs - 1);
    sx = min((int)(((long)rx * w.Ws) / w.Wo), w.Ws - 1);
}

__device__ __forceinline__ void hue_shift(float v[3], float h) {
    const float R = v[0], G = v[1], B = v[2];
    const float mx = fmaxf(R, fmaxf(G, B)), mn = fminf(R, fminf(G, B)), d = mx - mn;
    const float S = mx > 0.f ? d / mx : 0.f;
    float H = 0.f;
    if (d > 0.f) {
        if (mx == R) { H = (G - B) / d; if (H < 0.f) H += 6.f; }
        else if (mx == G) H = (B - R) / d + 2.f;
        else H = (R - G) / d + 4.f;
        H = H / 6.f;
    }
    H = H + h;
    H = H - floorf(H);
    const float H6 = H * 6.f, fi = floorf(H6), f = H6 - fi;
    const int i = ((int)fi) % 6;
    const float p = mx * (1.f - S), q = mx * (1.f - f * S), t = mx * (1.f - (1.f - f) * S);
    float r, g, b;
    if (i == 0) { r = mx; g = t; b = p; }
    else if (i == 1) { r = q; g = mx; b = p; }
    else if (i == 2) { r = p; g = mx; b = t; }
    else if (i == 3) { r = p; g = q; b = mx; }
    else if (i == 4) { r = t; g = p; b = mx; }
    else { r = mx; g = p; b = q; }
    v[0] = clip255(rintf(r)); v[1] = clip255(rintf(g)); v[2] = clip255(rintf(b));
}

// the pointwise ops [i0, i1) of the program at working-frame pixel (y, x); GRID and BLUR never lie inside the range
__device__ __forceinline__ void pointwise(const View& w, int i0, int i1, int y, int x, float v[3]) {
    const long pix = (long)y * w.Wo + x, per = (long)w.Ho * w.Wo;
    for (int i = i0; i < i1; ++i) {
        const int op = w.row->op[i];
        const float a = w.row->a[i], b = w.row->b[i];
        if (op == UAPS_AUG_BC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // RandomBrightnessContrast on uint8: lut[v] = uint8(clip(v * alpha + beta * 255, 0, 255))  (truncation)
                float t = v[c] * a + b * 255.f;
                t = fminf(fmaxf(t, 0.f), 255.f);
                v[c] = (float)(int)t;
            }
        } else if (op == UAPS_AUG_NOISE) {
            U4 rnd;
            if (!w.noise) rnd = philox4x32_10(w.ctr + (uint64_t)pix, w.seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= w.Cs) break;
                float g;
                if (w.noise) {
                    g = w.noise[c * per + pix];
                } else {                                      // Box-Muller on two Philox words per channel pair
                    const float u1 = fmaxf(u01(pick(rnd, c & 1 ? 2 : 0)), 1e-7f), u2 = u01(pick(rnd, c & 1 ? 3 : 1));
                    const float rad = sqrtf(-2.f * __logf(u1));
                    g = (c == 2 ? rad * __sinf(6.2831853f * u2) : rad * __cosf(6.2831853f * u2)) * a;
                }
                v[c] = (float)(int)fminf(fmaxf(v[c] + g, 0.f), 255.f);  // float32 add, clip, astype(uint8) truncates
            }
            if (w.Cs == 1) v[1] = v[2] = v[0];
        } else if (op == UAPS_AUG_BRIGHT) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (float)(int)clip255(v[c] * a);
        } else if (op == UAPS_AUG_CONTRAST) {
            const float shift = w.m * (1.f - a);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (float)(int)clip255(v[c] * a + shift);
        } else if (op == UAPS_AUG_SATURATE) {
            if (w.Cs == 3) {
                const float grey = 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2];
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = rintf(clip255(grey + a * (v[c] - grey)));
            }
        } else if (op == UAPS_AUG_HUE) {
            if (w.Cs == 3) hue_shift(v, a);
        } else if (op == UAPS_AUG_PIXDROP) {
            float u;
            if (w.drop) u = w.drop[pix];
            else u = u01(philox4x32_10(w.ctr + (uint64_t)pix, w.seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1)).x);
            if (u < a) v[0] = v[1] = v[2] = 0.f;
        }
    }
}

// a one-channel source is carried as three equal channels (every op keeps them equal)
__device__ __forceinline__ void level0(const View& w, int y, int x, int n, float v[3]) {
    int sy, sx;
    source_of(w, y, x, sy, sx);
    const uint8_t* p = w.src + ((long)sy * w.Ws + sx) * w.Cs;
    if (w.Cs == 3) { v[0] = (float)p[0]; v[1] = (float)p[1]; v[2] = (float)p[2]; }
    else v[0] = v[1] = v[2] = (float)p[0];
    pointwise(w, 0, n, y, x, v);
}

// position along a grid map -> the two reflect-101 nodes and the weight of the second
__device__ __forceinline__ void grid_nodes(float pos, int n, int& i0, int& i1, float& wt) {
    pos = fminf(fmaxf(pos, 0.f), (float)(n - 1));           // also maps NaN to 0: the indices below stay inside the frame
    const float f = floorf(pos);
    i0 = (int)f; wt = pos - f;
    i1 = reflect101(i0 + 1, n);
}

__device__ __forceinline__ void level1(const View& w, int y, int x, int n, float v[3]) {
    if (w.g < 0 || w.g >= n) { level0(w, y, x, n, v); return; }
    int y0, y1, x0, x1; float wy, wx;
    grid_nodes(w.gys[y], w.Ho, y0, y1, wy);
    grid_nodes(w.gxs[x], w.Wo, x0, x1, wx);
    float v00[3], v01[3], v10[3], v11[3];
    level0(w, y0, x0, w.g, v00); level0(w, y0, x1, w.g, v01);
    level0(w, y1, x0, w.g, v10); level0(w, y1, x1, w.g, v11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (1.f - wx) * v00[c] + wx * v01[c], bot = (1.f - wx) * v10[c] + wx * v11[c];
        v[c] = clip255(rintf((1.f - wy) * top + wy * bot));
    }
    pointwise(w, w.g + 1, n, y, x, v);
}

__device__ __forceinline__ void level2(const View& w, int y, int x, int n, float v[3]) {
    if (w.k < 0 || w.k >= n) { level1(w, y, x, n, v); return; }
    const int r = w.r;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int dy = -r; dy <= r; ++dy) {
        const int yy = reflect101(y + dy, w.Ho);
        for (int dx = -r; dx <= r; ++dx) {
            const int xx = reflect101(x + dx, w.Wo);
            float t[3];
            level1(w, yy, xx, w.k, t);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += t[c];   // integers below 2^24: exact in any order
        }
    }
    const float inv = 1.f / (float)((2 * r + 1) * (2 * r + 1));
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = rintf(acc[c] * inv);   // cv2.blur on uint8 rounds half to even
    pointwise(w, w.k + 1, n, y, x, v);
}

// thread -> (view, pixel): a workgroup holds 256 / V consecutive pixels of ONE image, view by view, so that both views of a
// pixel run on one compute unit (the source lines are fetched from HBM once) while every wavefront belongs to one view (its
// program is wave-uniform) and stores 64 consecutive x per channel plane.
__device__ __forceinline__ bool locate(const Args& a, int& v, long& pix) {
    const int P = kThreads / a.V;
    v = __builtin_amdgcn_readfirstlane((int)threadIdx.x / P);
    pix = (long)blockIdx.x * P + ((int)threadIdx.x - v * P);
    return pix < (long)a.Ho * a.Wo;
}

__global__ __launch_bounds__(kThreads) void views_kernel(Args a) {
    int v; long pix;
    if (!locate(a, v, pix)) return;
    const int b = blockIdx.y;
    View w = make_view(a, v, b);
    const long vb = (long)v * a.B + b, per = (long)a.Ho * a.Wo;
    if (w.c >= 0 && a.m) w.m = a.m[vb];
    const int y = (int)(pix / a.Wo), x = (int)(pix % a.Wo);
    float val[3];
    level2(w, y, x, w.nops, val);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= a.Cs) break;
        a.out[(vb * a.Cs + c) * per + pix] = (val[c] / 255.f - a.mean[c]) / a.stdv[c];
    }
    if (a.masks && a.out_mask) {
        int my = y, mx = x;
        if (w.g >= 0) {                                       // the node nearest to the grid position
            my = (int)rintf(fminf(fmaxf(w.gys[y], 0.f), (float)(a.Ho - 1)));
            mx = (int)rintf(fminf(fmaxf(w.gxs[x], 0.f), (float)(a.Wo - 1)));
        }
        int sy, sx;
        source_of(w, my, mx, sy, sx);
        a.out_mask[vb * per + pix] = (int64_t)a.masks[((long)b * a.Hs + sy) * a.Ws + sx];
    }
}

// CONTRAST pre-pass, stage 1: grey levels x 1000 (integers) of the image entering the op, one partial sum per workgroup.
// blockIdx.y = view * B + image; a (view, image) without CONTRAST leaves at once.
__global__ __launch_bounds__(kThreads) void contrast_partial_kernel(Args a, int blocks_per_frame) {
    __shared__ uint32_t red[kThreads];
    const int vb = blockIdx.y, v = vb / a.B, b = vb - v * a.B;
    View w = make_view(a, v, b);
    if (w.c < 0) return;
    const long pix = (long)blockIdx.x * kThreads + threadIdx.x;
    uint32_t g = 0;
    if (pix < (long)a.Ho * a.Wo) {
        float val[3];
        level2(w, (int)(pix / a.Wo), (int)(pix % a.Wo), w.c, val);
        g = a.Cs == 3 ? 299u * (uint32_t)val[0] + 587u * (uint32_t)val[1] + 114u * (uint32_t)val[2] : 1000u * (uint32_t)val[0];
    }
    red[threadIdx.x] = g;                                     // <= 256 * 255000 < 2^32
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.partial[(long)vb * blocks_per_frame + blockIdx.x] = red[0];
}

// stage 2: the partials of one (view, image) in a fixed order; m = rint(sum / (1000 * Ho * Wo)), -1 without CONTRAST
__global__ __launch_bounds__(kThreads) void contrast_final_kernel(Args a, int blocks_per_frame) {
    __shared__ unsigned long long red[kThreads];
    const int vb = blockIdx.x, v = vb / a.B, b = vb - v * a.B;
    const View w = make_view(a, v, b);
    if (w.c < 0) { if (threadIdx.x == 0) a.m[vb] = -1.f; return; }
    unsigned long long s = 0;
    for (int i = threadIdx.x; i < blocks_per_frame; i += kThreads) s += a.partial[(long)vb * blocks_per_frame + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.m[vb] = (float)rint((double)red[0] / (1000.0 * (double)a.Ho * (double)a.Wo));
}

inline long frame_blocks(int Ho, int Wo) { return ((long)Ho * Wo + kThreads - 1) / kThreads; }
}  // namespace

extern "C" int uaps_augment_views_workspace_bytes(int V, int B, int Ho, int Wo, size_t* bytes) {
    if (!bytes || (V != 1 && V != 2) || B <= 0 || Ho <= 0 || Wo <= 0) return UAPS_EINVAL;
    if ((long)V * B > 65535 || (long)Ho * Wo > 0x7fffffffL) return UAPS_ERANGE;
    *bytes = (size_t)V * B * (1 + (size_t)frame_blocks(Ho, Wo)) * 4;
    return UAPS_OK;
}

extern "C" int uaps_augment_views(const uaps_augment_views_call* call) {
    uaps_augment_views_call c;                  // (this entry point also refuses a struct longer than its own)
    if (uaps::read_call(call, c) || call->struct_size > sizeof c) return UAPS_EINVAL;
    if (!c.images || !c.rows_host || !c.rows || !c.out || (c.masks != nullptr) != (c.out_mask != nullptr)) return UAPS_EINVAL;
    if ((c.V != 1 && c.V != 2) || (c.Cs != 1 && c.Cs != 3) || c.B <= 0 || c.Hs <= 0 || c.Ws <= 0 || c.Ho <= 0 || c.Wo <= 0) return UAPS_EINVAL;
    if ((long)c.V * c.B > 65535 || (long)c.Ho * c.Wo > 0x7fffffffL || (long)c.Hs * c.Ws > 0x7fffffffL) return UAPS_ERANGE;
    for (int ch = 0; ch < c.Cs; ++ch)
        if (!(c.std[ch] != 0.f)) return UAPS_EINVAL;
    bool any_contrast = false;
    int noform = 0;
    for (long i = 0; i < (long)c.V * c.B; ++i) {
        const uaps_view_row& r = c.rows_host[i];
        if (r.rot_k < 0 || r.rot_k > 3 || ((r.rot_k & 1) && c.Ho != c.Wo)) return UAPS_EINVAL;
        int grids = 0, blurs = 0, contrasts = 0;
        for (int j = 0; j < kMaxOps; ++j) {
            const int op = r.op[j];
            if (op == UAPS_AUG_END) break;
            if (op < 0 || op > UAPS_AUG_GRID) return UAPS_EINVAL;
            if (op == UAPS_AUG_BLUR) {
                if (r.a[j] != 3.f && r.a[j] != 5.f && r.a[j] != 7.f) return UAPS_EINVAL;
                ++blurs;
            }
            if (op == UAPS_AUG_GRID) {
                // the pixels in front of GRID are needed at four other places: no drawn field there, no window
                for (int q = 0; q < j; ++q)
                    if (r.op[q] == UAPS_AUG_NOISE || r.op[q] == UAPS_AUG_PIXDROP || r.op[q] == UAPS_AUG_BLUR) noform = 1;
                ++grids;
            }
            if (op == UAPS_AUG_CONTRAST) ++contrasts;
        }
        if (grids > 1 || blurs > 1 || contrasts > 1) noform = 1;
        if ((r.grid_on != 0) != (grids > 0)) return UAPS_EINVAL;
        if (grids && (!c.grid_ys || !c.grid_xs)) return UAPS_EINVAL;
        any_contrast |= contrasts > 0;
    }
    if (noform) return UAPS_ENOFORM;
    const long fb = frame_blocks(c.Ho, c.Wo);
    const long main_blocks = ((long)c.Ho * c.Wo + kThreads / c.V - 1) / (kThreads / c.V);
    if (any_contrast) {
        size_t need = 0;
        uaps_augment_views_workspace_bytes(c.V, c.B, c.Ho, c.Wo, &need);
        if (!c.workspace || c.workspace_bytes < need) return UAPS_EWORKSPACE;
    }
    Args a;
    a.V = c.V; a.B = c.B; a.Hs = c.Hs; a.Ws = c.Ws; a.Cs = c.Cs; a.Ho = c.Ho; a.Wo = c.Wo;
    a.images = c.images; a.masks = c.masks; a.rows = c.rows; a.grid_ys = c.grid_ys; a.grid_xs = c.grid_xs;
    a.noise = c.noise; a.drop_u = c.drop_u; a.seed = c.seed;
    for (int ch = 0; ch < 3; ++ch) { a.mean[ch] = c.mean[ch]; a.stdv[ch] = c.std[ch]; }
    a.out = c.out; a.out_mask = c.out_mask;
    a.m = any_contrast ? (float*)c.workspace : nullptr;
    a.partial = any_contrast ? (uint32_t*)c.workspace + (size_t)c.V * c.B : nullptr;
    hipStream_t s = (hipStream_t)c.stream;
    if (any_contrast) {
        hipLaunchKernelGGL(contrast_partial_kernel, dim3((unsigned)fb, (unsigned)(c.V * c.B)), dim3(kThreads), 0, s, a, (int)fb);
        hipLaunchKernelGGL(contrast_final_kernel, dim3((unsigned)(c.V * c.B)), dim3(kThreads), 0, s, a, (int)fb);
    }
    hipLaunchKernelGGL(views_kernel, dim3((unsigned)main_blocks, (unsigned)c.B), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}
