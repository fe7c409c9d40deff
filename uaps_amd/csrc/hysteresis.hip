// Hysteresis thresholding of score maps and binary reconstruction of label maps for gfx950 (include/uaps_hip.h, uaps_hysteresis):
// keep a connected region of candidate pixels only if it holds a seed.
//
// Five launches in one call, no host synchronisation; every launch boundary is the coherence point for the next:
//   1 classify_scores_kernel<C> / classify_markers_kernel
//                        writes the int64 CODE MAP into the workspace: class + 1 in the low word (0: the pixel forms nothing), the
//                        seed in bit 32.  Score form: all C scores of a pixel in registers, softmax (C == 1: sigmoid) with
//                        from_logits, the arg-max over the SELECTED classes alone, the two fp32 comparisons against that class's
//                        low and high.  Marker form: a pixel of a selected class of `mask`, the seed from `markers`.
//   2 hyst_tile_kernel   cc_tile_label on the code map: ONE labelling over the B images serves all classes (key = the low word).
//   3 hyst_seam_kernel   cc_seam_merge, the same policy.
//   4 hyst_flatten_kernel
//                        cc_flatten_area, in place (roots == parent), with the mark policy "bit 32 of the pixel's code": a seed
//                        raises bit 31 of its root's area word, on whichever of the pass's two send paths its run travels.
//   5 apply_kernel       a pixel with a code looks up the word of its root -- area in bits 0..30, "holds a seed" in bit 31 -- and
//                        writes its class or the background; every other pixel writes the background (score form) or its own
//                        value of `mask` (marker form).  `out` is written once.
// The workspace holds the code map (8 bytes a pixel) and the parent / root and area words (4 + 4).  The area words are zeroed by the
// tile pass of every call: nothing survives from an earlier call or whoever owned the workspace before.  Integer atomics only
// (atomicMin, atomicAdd, atomicOr): two runs give the same bits.  No workgroup waits for another inside a launch; every flat index
// over B * C * H * W is 64-bit.
#include <stdint.h>
#include <string.h>
#include "cc_common.hpp"
#include "loss_common.hpp"               // uaps::pixel: the scores of a pixel in registers, their softmax

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256;
using namespace uaps::cc;

constexpr int kMaxClasses = UAPS_HYST_MAX_CLASSES;
constexpr int kMaxGrid = 1 << 24;
constexpr long long kSeedBit = 1ll << 32;

// components of equal low words of the code map; a zero low word forms nothing
struct CodePolicy {
    __device__ __forceinline__ int image(int q) const { return q; }
    __device__ __forceinline__ bool fg(long long v, int) const { return (unsigned)v != 0u; }
    __device__ __forceinline__ long long key(long long v, int) const { return (long long)(unsigned)v; }
};
// the seed bit of the pixel's code
struct SeedMark {
    static constexpr bool kOn = true;
    const long long* code;
    __device__ __forceinline__ bool operator()(long n, long) const { return (code[n] & kSeedBit) != 0; }
};
using CodeArgs = CcArgs<CodePolicy>;

struct ClassifyArgs {
    long N, HW;                 // N = B * HW pixels
    int nc, from_logits;
    int cls[kMaxClasses];       // ascending
    float low[kMaxClasses], high[kMaxClasses];
    const float* S;             // [B][C][H][W]
    const long long* mask;      // [B][H][W]
    const uint8_t* markers;     // [B][H][W]
    long long* code;            // [B][H][W]
};

template <int C>
__global__ __launch_bounds__(kThreads) void classify_scores_kernel(ClassifyArgs a) {
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < a.N; n += (long)gridDim.x * kThreads) {
        const long b = n / a.HW, i = n - b * a.HW;
        float z[C][1];
        uaps::pixel::load_logits<C, 1>(a.S + b * C * a.HW + i, a.HW, z);
        if (a.from_logits) {
            if constexpr (C == 1) {
                z[0][0] = 1.f / (1.f + expf(-z[0][0]));
            } else {
                float mx[1], lse[1];
                uaps::pixel::softmax_inplace<C, 1>(z, mx, lse);
            }
        }
        // the arg-max over the selected classes (ascending, strict >: the lowest class among equal scores) with that class's
        // thresholds carried along: k is uniform, nothing is indexed by a lane's own value
        float best = 0.f, lo = 0.f, hi = 0.f;
        int c = -1;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < kMaxClasses; ++k) {
            if (k < a.nc) {
                const float s = C == 1 ? z[0][0] : uaps::pixel::pick<C, 1>(z, 0, a.cls[k]);
                bad = bad || s != s;
                if (c < 0 || s > best) { best = s; c = a.cls[k]; lo = a.low[k]; hi = a.high[k]; }
            }
        }
        long long code = 0;
        if (!bad && c >= 0 && best >= lo) code = (long long)(c + 1) | (best >= hi ? kSeedBit : 0ll);
        a.code[n] = code;
    }
}

__global__ __launch_bounds__(kThreads) void classify_markers_kernel(ClassifyArgs a) {
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < a.N; n += (long)gridDim.x * kThreads) {
        const long long v = a.mask[n];
        bool sel = false;
#pragma unroll
        for (int k = 0; k < kMaxClasses; ++k) sel = sel || (k < a.nc && v == (long long)a.cls[k]);
        a.code[n] = sel ? ((v + 1) | (a.markers[n] != 0 ? kSeedBit : 0ll)) : 0ll;
    }
}

__global__ __launch_bounds__(kThreads) void hyst_tile_kernel(CodeArgs a) {
    __shared__ long long cls[kTile];
    __shared__ int lab[kTile];
    cc_tile_label(a, cls, lab);
}
__global__ __launch_bounds__(kThreads) void hyst_seam_kernel(CodeArgs a) { cc_seam_merge(a); }

// in place: words[n] parent -> root (cc_common.hpp, cc_flatten_area, on why that is sound)
__global__ __launch_bounds__(kThreads) void hyst_flatten_kernel(int* words, int* area, const long long* code, long HW, long N) {
    cc_flatten_area(words, words, area, HW, N, SeedMark{code});
}

struct ApplyArgs {
    long N, HW;
    int min_area;
    long long bg;
    const long long* code;
    const long long* mask;      // marker form; NULL in the score form
    long long* out;
    const int* root;            // [B][HW]
    const int* area;            // [B][HW]: at a root, area | kBorderBit where the component holds a seed
};

__global__ __launch_bounds__(kThreads) void apply_kernel(ApplyArgs a) {
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < a.N; n += (long)gridDim.x * kThreads) {
        const unsigned cw = (unsigned)a.code[n];
        long long o = a.bg;
        if (cw != 0u) {                         // (a code, so a foreground pixel of the labelling: it has a root)
            const long b = n / a.HW;
            const unsigned w = (unsigned)a.area[b * a.HW + a.root[n]];
            if ((w & kBorderBit) != 0u && (int)(w & kAreaMask) >= a.min_area) o = (long long)cw - 1;
        } else if (a.mask) {
            o = a.mask[n];
        }
        a.out[n] = o;
    }
}

inline int grid_of(long items) { return grid_for(items, kMaxGrid); }

inline int check_dims(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if ((double)H * W >= kTooBig || (double)B * H * W * 8.0 >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}
// the code map, the parent / root words and the area words
inline double workspace_size(int B, int H, int W) { return (double)B * H * W * 16.0 + 3 * 256.0; }
inline size_t workspace_for(int B, int H, int W) {
    const size_t N = (size_t)B * H * W;
    return align256(8 * N) + 2 * align256(4 * N);
}

template <int C>
void launch_classify(const ClassifyArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(classify_scores_kernel<C>, dim3(grid_of(a.N)), dim3(kThreads), 0, st, a);
}
}  // namespace

extern "C" int uaps_hysteresis_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    const int rc = check_dims(B, H, W);
    if (rc) return rc;
    if (workspace_size(B, H, W) >= kTooBig) return UAPS_ERANGE;
    *bytes = workspace_for(B, H, W);
    return UAPS_OK;
}

extern "C" int uaps_hysteresis(const uaps_hysteresis_call* call) {
    uaps_hysteresis_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    const bool score = c.scores != nullptr;
    if (!c.out || !c.workspace) return UAPS_EINVAL;
    if (score ? (c.mask || c.markers) : (!c.mask || !c.markers || c.out == c.mask)) return UAPS_EINVAL;
    int rc = check_dims(c.B, c.H, c.W);
    if (rc == UAPS_EINVAL) return rc;
    if (c.n_classes < 1 || c.n_classes > kMaxClasses) return UAPS_EINVAL;
    for (int k = 0; k < c.n_classes; ++k) {
        if (c.classes[k] < 0 || c.classes[k] == INT32_MAX || c.classes[k] == c.background) return UAPS_EINVAL;
        if (k > 0 && c.classes[k] <= c.classes[k - 1]) return UAPS_EINVAL;
    }
    if ((c.connectivity != 4 && c.connectivity != 8) || c.min_area < 1) return UAPS_EINVAL;
    if (score) {
        if (c.from_logits != 0 && c.from_logits != 1) return UAPS_EINVAL;
        if (c.C < 1 || c.C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
        for (int k = 0; k < c.n_classes; ++k) {
            if (c.C == 1 ? c.classes[k] != 1 : c.classes[k] >= c.C) return UAPS_EINVAL;
            if (!(c.low[k] <= c.high[k])) return UAPS_EINVAL;          // (false for a NaN on either side)
        }
    }
    if (rc) return rc;
    if (score && (double)c.B * c.C * c.H * c.W * 4.0 >= kTooBig) return UAPS_ERANGE;
    if (workspace_size(c.B, c.H, c.W) >= kTooBig) return UAPS_ERANGE;
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, workspace_for(c.B, c.H, c.W))) return UAPS_EWORKSPACE;

    const long HW = (long)c.H * c.W, N = (long)c.B * HW;
    char* ws = static_cast<char*>(c.workspace);
    long long* code = reinterpret_cast<long long*>(ws);
    int* parent = reinterpret_cast<int*>(ws + align256(8 * (size_t)N));
    int* area = reinterpret_cast<int*>(ws + align256(8 * (size_t)N) + align256(4 * (size_t)N));
    hipStream_t st = (hipStream_t)c.stream;
    uaps::account_bytes((double)N * (score ? 4.0 * c.C + 8.0 : 8.0 + 1.0 + 8.0));

    ClassifyArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.N = N; ca.HW = HW; ca.nc = c.n_classes; ca.from_logits = c.from_logits;
    for (int k = 0; k < c.n_classes; ++k) { ca.cls[k] = c.classes[k]; ca.low[k] = c.low[k]; ca.high[k] = c.high[k]; }
    ca.S = c.scores; ca.mask = (const long long*)c.mask; ca.markers = c.markers; ca.code = code;
    if (score) {
        switch (c.C) {
            case 1: launch_classify<1>(ca, st); break;
            case 2: launch_classify<2>(ca, st); break;
            case 3: launch_classify<3>(ca, st); break;
            case 4: launch_classify<4>(ca, st); break;
            case 5: launch_classify<5>(ca, st); break;
            case 6: launch_classify<6>(ca, st); break;
            case 7: launch_classify<7>(ca, st); break;
            default: launch_classify<8>(ca, st); break;
        }
    } else {
        hipLaunchKernelGGL(classify_markers_kernel, dim3(grid_of(N)), dim3(kThreads), 0, st, ca);
    }

    CodeArgs a;
    memset(&a, 0, sizeof a);
    a.Q = c.B; a.H = c.H; a.W = c.W; a.ntx = (c.W + kTW - 1) / kTW; a.nty = (c.H + kTH - 1) / kTH;
    a.conn8 = c.connectivity == 8 ? 1 : 0; a.mask = code; a.parent = parent; a.area = area;
    const long tiles = (long)c.B * a.ntx * a.nty;               // < 2^31: the workspace bound keeps B * HW below 2^27
    const long seam = (long)c.B * ((long)(a.nty - 1) * c.W + (long)(a.ntx - 1) * c.H);
    hipLaunchKernelGGL(hyst_tile_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, a);
    if (seam > 0) hipLaunchKernelGGL(hyst_seam_kernel, dim3(grid_of(seam)), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(hyst_flatten_kernel, dim3(span_grid(N)), dim3(kThreads), 0, st, parent, area, (const long long*)code, HW, N);

    ApplyArgs ap;
    memset(&ap, 0, sizeof ap);
    ap.N = N; ap.HW = HW; ap.min_area = c.min_area; ap.bg = c.background; ap.code = code;
    ap.mask = score ? nullptr : (const long long*)c.mask; ap.out = (long long*)c.out; ap.root = parent; ap.area = area;
    UAPS_LAUNCH_MAIN(apply_kernel, dim3(grid_of(N)), dim3(kThreads), 0, st, ap);
    return (int)hipGetLastError();
}
