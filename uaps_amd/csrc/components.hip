// Component clean-up of a label map for gfx950 (include/uaps_hip.h, uaps_components): area opening, clear border, hole filling.
//
// A chain of 1..8 steps, each reading the map the previous one wrote, in one call without a host synchronisation.  Every step is the
// three labelling launches of cc_common.hpp (tile-local union-find in LDS, seam merge with agent-scope atomicMin, flatten + area with
// the border flag) and one apply pass that writes the step's map once.  Nothing is numbered: no scan.
//
//   area_open n / clear_border   ONE labelling over the B images serves all classes: equal values belong together under the call's
//                                connectivity, the background forms nothing.  apply_fg_kernel: a pixel of a selected class looks up
//                                the word of its root -- area in bits 0..30, "touches the border" in bit 31 -- and writes the
//                                background or its own value; every other pixel is copied.
//   fill_holes n                 B * n_classes VIRTUAL planes, plane q = b * n_classes + p: the foreground is mask[b] != classes[p]
//                                (read from the map; no one-hot tensor exists), connected under the COMPLEMENTARY connectivity.  A
//                                component without the border bit is a hole of classes[p].  apply_holes_kernel: a background pixel
//                                walks the planes in ascending class order and takes the first class whose root word there has no
//                                border bit and an area <= n; every other pixel is copied.
//
// The flatten pass stores every pixel's root over its parent word (roots == parent), so the workspace holds two words per pixel and
// plane: parent / root and area.  The area words are zeroed by the tile pass of EVERY step; nothing survives from an earlier step, an
// earlier call or whoever owned the workspace before.  Integer atomics only (atomicMin, atomicAdd, atomicOr): two runs give the same
// bits.  No workgroup waits for another inside a launch; every flat index over B * n_classes * H * W is 64-bit.
#include <stdint.h>
#include <string.h>
#include "cc_common.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256;
using namespace uaps::cc;

constexpr int kMaxClasses = UAPS_COMP_MAX_CLASSES, kMaxSteps = UAPS_COMP_MAX_STEPS;
constexpr int kMaxGrid = 1 << 24;

// cls[p] for a p that differs from lane to lane: a chain of selects (an indexed read of a by-value array would go through scratch)
__device__ __forceinline__ long long pick(const long long (&cls)[kMaxClasses], int p) {
    long long c = cls[0];
#pragma unroll
    for (int k = 1; k < kMaxClasses; ++k) c = p == k ? cls[k] : c;
    return c;
}

// plane q = b * n + p: everything that is not classes[p], as one kind of pixel
struct ComplementPolicy {
    int n;
    long long cls[kMaxClasses];
    __device__ __forceinline__ int image(int q) const { return q / n; }
    __device__ __forceinline__ bool fg(long long v, int q) const { return v != pick(cls, q % n); }
    __device__ __forceinline__ long long key(long long, int) const { return 0; }
};

using FgArgs = CcArgs<SameValuePolicy>;
using HoleArgs = CcArgs<ComplementPolicy>;

__global__ __launch_bounds__(kThreads) void comp_tile_fg_kernel(FgArgs a) {
    __shared__ long long cls[kTile];
    __shared__ int lab[kTile];
    cc_tile_label(a, cls, lab);
}
__global__ __launch_bounds__(kThreads) void comp_tile_holes_kernel(HoleArgs a) {
    __shared__ long long cls[kTile];
    __shared__ int lab[kTile];
    cc_tile_label(a, cls, lab);
}
__global__ __launch_bounds__(kThreads) void comp_seam_fg_kernel(FgArgs a) { cc_seam_merge(a); }
__global__ __launch_bounds__(kThreads) void comp_seam_holes_kernel(HoleArgs a) { cc_seam_merge(a); }

// in place: words[n] parent -> root (cc_common.hpp, cc_flatten_area, on why that is sound)
__global__ __launch_bounds__(kThreads) void comp_flatten_kernel(int* words, int* area, long HW, long N, int H, int W) {
    cc_flatten_area(words, words, area, HW, N, BorderMark{H, W});
}

struct ApplyArgs {
    long N, HW;                 // N = B * HW pixels of the map
    int nc, kind, limit;
    long long cls[kMaxClasses]; // ascending
    long long bg;
    const long long* in;
    long long* out;
    const int* root;            // [planes][HW]
    const int* area;            // [planes][HW]: at a root, area | kBorderBit
};

__global__ __launch_bounds__(kThreads) void apply_fg_kernel(ApplyArgs a) {
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < a.N; n += (long)gridDim.x * kThreads) {
        const long long v = a.in[n];
        bool sel = false;
#pragma unroll
        for (int k = 0; k < kMaxClasses; ++k) sel = sel || (k < a.nc && v == a.cls[k]);
        long long o = v;
        if (sel) {                              // (selected, so not the background: the pixel has a root)
            const long b = n / a.HW;
            const unsigned w = (unsigned)a.area[b * a.HW + a.root[n]];
            const bool drop = a.kind == UAPS_COMP_AREA_OPEN ? (int)(w & kAreaMask) < a.limit : (w & kBorderBit) != 0u;
            if (drop) o = a.bg;
        }
        a.out[n] = o;
    }
}

__global__ __launch_bounds__(kThreads) void apply_holes_kernel(ApplyArgs a) {
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < a.N; n += (long)gridDim.x * kThreads) {
        const long long v = a.in[n];
        long long o = v;
        if (v == a.bg) {                        // (the background is no selected class: foreground in every plane)
            const long b = n / a.HW, i = n - b * a.HW;
            bool done = false;
#pragma unroll
            for (int p = 0; p < kMaxClasses; ++p) {
                if (p < a.nc && !done) {
                    const long q = (b * a.nc + p) * a.HW;
                    const unsigned w = (unsigned)a.area[q + a.root[q + i]];
                    if (!(w & kBorderBit) && (int)(w & kAreaMask) <= a.limit) { o = a.cls[p]; done = true; }
                }
            }
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
// parent / root and area words of `planes` planes an image, and the map between two steps
inline double workspace_size(int B, int H, int W, int planes) { return (double)B * H * W * (8.0 * planes + 8.0) + 3 * 256.0; }
inline size_t workspace_for(int B, int H, int W, int planes) {
    const size_t N = (size_t)B * H * W;
    return 2 * align256(4 * N * planes) + align256(8 * N);
}

template <typename Args>
inline void fill_args(Args& a, const uaps_components_call& c, int planes, bool conn8, const long long* in, int* parent, int* area) {
    a.Q = c.B * planes; a.H = c.H; a.W = c.W; a.ntx = (c.W + kTW - 1) / kTW; a.nty = (c.H + kTH - 1) / kTH;
    a.conn8 = conn8 ? 1 : 0; a.mask = in; a.parent = parent; a.area = area;
}
}  // namespace

extern "C" int uaps_components_workspace_bytes(int B, int H, int W, int n_classes, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    const int rc = check_dims(B, H, W);
    if (rc) return rc;
    if (n_classes < 1 || n_classes > kMaxClasses) return UAPS_EINVAL;
    if (workspace_size(B, H, W, n_classes) >= kTooBig) return UAPS_ERANGE;
    *bytes = workspace_for(B, H, W, n_classes);
    return UAPS_OK;
}

extern "C" int uaps_components(const uaps_components_call* call) {
    uaps_components_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.mask || !c.out || !c.workspace || c.out == c.mask) return UAPS_EINVAL;
    int rc = check_dims(c.B, c.H, c.W);
    if (rc == UAPS_EINVAL) return rc;
    if (c.n_steps < 1 || c.n_steps > kMaxSteps) return UAPS_EINVAL;
    bool holes = false;
    for (int s = 0; s < c.n_steps; ++s) {
        const int k = c.kind[s];
        if (k != UAPS_COMP_AREA_OPEN && k != UAPS_COMP_CLEAR_BORDER && k != UAPS_COMP_FILL_HOLES) return UAPS_EINVAL;
        if (k != UAPS_COMP_CLEAR_BORDER && c.n[s] < 1) return UAPS_EINVAL;
        holes = holes || k == UAPS_COMP_FILL_HOLES;
    }
    if (c.n_classes < 1 || c.n_classes > kMaxClasses) return UAPS_EINVAL;
    if (!uaps::distinct_classes(c.classes, c.n_classes, c.background)) return UAPS_EINVAL;
    if (c.connectivity != 4 && c.connectivity != 8) return UAPS_EINVAL;
    if (rc) return rc;
    const int planes = holes ? c.n_classes : 1;
    if (workspace_size(c.B, c.H, c.W, planes) >= kTooBig) return UAPS_ERANGE;
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, workspace_for(c.B, c.H, c.W, planes))) return UAPS_EWORKSPACE;

    const long HW = (long)c.H * c.W, N = (long)c.B * HW;
    char* ws = static_cast<char*>(c.workspace);
    int* parent = reinterpret_cast<int*>(ws);
    int* area = reinterpret_cast<int*>(ws + align256(4 * (size_t)N * planes));
    long long* tmp = reinterpret_cast<long long*>(ws + 2 * align256(4 * (size_t)N * planes));
    hipStream_t st = (hipStream_t)c.stream;
    uaps::account_bytes(16.0 * (double)N);

    ApplyArgs ap;
    memset(&ap, 0, sizeof ap);
    ap.N = N; ap.HW = HW; ap.nc = c.n_classes; ap.bg = c.background; ap.root = parent; ap.area = area;
    for (int k = 0; k < c.n_classes; ++k) ap.cls[k] = c.classes[k];
    for (int k = 1; k < c.n_classes; ++k)       // ascending: the smallest class wins a shared hole
        for (int j = k; j > 0 && ap.cls[j - 1] > ap.cls[j]; --j) { const long long t = ap.cls[j]; ap.cls[j] = ap.cls[j - 1]; ap.cls[j - 1] = t; }

    const long long* in = (const long long*)c.mask;
    for (int s = 0; s < c.n_steps; ++s) {
        long long* out = ((c.n_steps - 1 - s) & 1) ? tmp : (long long*)c.out;      // the last step writes `out`
        const bool fill = c.kind[s] == UAPS_COMP_FILL_HOLES;
        const int np = fill ? c.n_classes : 1;
        const int ntx = (c.W + kTW - 1) / kTW, nty = (c.H + kTH - 1) / kTH;
        const long tiles = (long)c.B * np * ntx * nty;             // < 2^31: the workspace bound keeps B * np * HW below 2^28
        const long seam = (long)c.B * np * ((long)(nty - 1) * c.W + (long)(ntx - 1) * c.H);
        if (fill) {
            HoleArgs a;
            memset(&a, 0, sizeof a);
            fill_args(a, c, np, c.connectivity == 4, in, parent, area);            // the complementary connectivity
            a.pol.n = np;
            for (int k = 0; k < kMaxClasses; ++k) a.pol.cls[k] = ap.cls[k];
            hipLaunchKernelGGL(comp_tile_holes_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, a);
            if (seam > 0) hipLaunchKernelGGL(comp_seam_holes_kernel, dim3(grid_of(seam)), dim3(kThreads), 0, st, a);
        } else {
            FgArgs a;
            memset(&a, 0, sizeof a);
            fill_args(a, c, 1, c.connectivity == 8, in, parent, area);
            a.pol.has_bg = 1; a.pol.bg = c.background;
            hipLaunchKernelGGL(comp_tile_fg_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, a);
            if (seam > 0) hipLaunchKernelGGL(comp_seam_fg_kernel, dim3(grid_of(seam)), dim3(kThreads), 0, st, a);
        }
        hipLaunchKernelGGL(comp_flatten_kernel, dim3(span_grid(N * np)), dim3(kThreads), 0, st, parent, area, HW, N * np, c.H, c.W);
        ap.kind = c.kind[s]; ap.limit = c.n[s]; ap.in = in; ap.out = out;
        if (fill) UAPS_LAUNCH_MAIN(apply_holes_kernel, dim3(grid_of(N)), dim3(kThreads), 0, st, ap);
        else UAPS_LAUNCH_MAIN(apply_fg_kernel, dim3(grid_of(N)), dim3(kThreads), 0, st, ap);
        in = out;
    }
    return (int)hipGetLastError();
}
