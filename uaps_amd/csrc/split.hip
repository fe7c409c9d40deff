// Splitting of touching defects for gfx950 (include/uaps_hip.h, uaps_split_instances): erode every defect to its cores (the MARKERS),
// grow the cores back inside the defect one pixel a round, cut where the fronts meet -- the geodesic zones of influence of the markers
// -- and number and tabulate the pieces the way uaps_label_instances does.  The result is a pure function of the input.
//
// One call, no host synchronisation, a launch count fixed by the arguments; every launch boundary is the coherence point of the next:
//   1 split_classify_kernel  the int64 MARKER CODE MAP into the workspace: the source label where labels > 0 and the pixel is a marker
//                            pixel (distance form: D >= d2; marker form: markers != 0), 0 elsewhere.  Resets the per-image words.
//   2 split_tile_kernel / split_seam_kernel / split_flatten_kernel
//                            cc_common.hpp's three labelling passes on that map, SameValuePolicy with the background 0: a marker is a
//                            component of equal codes; its root word names its first pixel, the root's area word its pixel count.
//   3 split_init_kernel      the int32 owner plane: root + 1 on the pixels of a marker of at least min_marker_area pixels, 0 elsewhere.
//   4 split_grow_kernel      ceil(max_iters / S) launches of S synchronous rounds.  A workgroup stages the source labels and the owners
//                            of `band` x `tw` owned pixels and a halo of S pixels (on every side along which the image has more than
//                            one tile) in LDS; a round lets every unowned defect pixel take the smallest owner among its neighbours of
//                            the same source label, all reads from the round's start (two owner buffers in LDS).  A round looks one
//                            pixel far: after round k only cells at least k from the staged tile's outer edge are exact, so round k
//                            forms only those, and after S rounds the owned cells are exact and are all a tile stores.  Global planes
//                            ping-pong between launches.  last[b] = 1 + the index of the last launch that gave an owned pixel of image
//                            b an owner (a plain store of that constant); launch L returns at once where last[b] < L: launch L - 1 made
//                            S >= 1 rounds and changed nothing, so the plane is a fixed point and BOTH planes hold it.  A tile whose
//                            round changed none of its cells stops its rounds early: every later round would change none either.
//   5 split_check_kernel     converged[b] := 0 where an unowned defect pixel has an owned neighbour of its source label.
//   6 split_code_kernel      the PIECE CODE MAP (label << 32) | owner over the marker code map's words.
//   7 uaps::label_launches   the launches of uaps_label_instances on that map (instances_launch.hpp): pieces are components of equal codes.
//   8 split_fixup_kernel     per table row: the class column, which holds the code, becomes the source defect's class (source_table;
//                            -1 for a source label without a row there), parent[k] the source label, pieces[source] += 1 (one integer
//                            atomic a piece).
// Integers only, no float, no scratch; two runs, every band height, tile width and S give the same bits.
#include <string.h>
#include "cc_common.hpp"
#include "instances_launch.hpp"

namespace {
using uaps::kThreads; using uaps::kTooBig; using uaps::grid_for; using uaps::align256;
using namespace uaps::cc;

constexpr int kMaxExtent = UAPS_SPLIT_MAX_EXTENT, kMaxS = UAPS_SPLIT_MAX_SUB_ITERS;
constexpr int kLdsCells = (64 * 1024 - 256) / 12;       // the budget of a workgroup: a label and two owners a staged cell, beside
                                                        // the 256 static bytes of the round's block-wide vote
constexpr int kDefaultS = 8;                    // rounds a launch (the S sweep)
constexpr int kDefaultCols = 32;                // owned columns of a tile
constexpr int kMaxGrid = 1 << 20;

using MarkArgs = CcArgs<SameValuePolicy>;

struct SplitArgs {
    int B, H, W, conn8;
    int d2, min_marker_area, M, Ms;         // M: rows of table / parent; Ms: rows of source_table / pieces
    int S, s_now, launch;                   // halo width, rounds of this launch, its index
    int band, tw, hy, hx, R, SW, nby, ntx;  // owned rows / columns, halo rows / columns (0 | S), staged rows / columns, tiles
    const int* labels;                      // the source labels [B][H][W]
    const int* distance;
    const unsigned char* markers;
    long long* code;                        // [B][H][W]
    const int* root;                        // the marker roots
    const int* area;
    const int* src;                         // owner planes
    int* dst;
    unsigned* last;                         // [B]
    unsigned char* converged;               // [B]
    const long long* source_table;
    long long* table;
    const int* count;
    int* parent;
    int* pieces;
};

__global__ __launch_bounds__(kThreads) void split_classify_kernel(SplitArgs a) {
    const long gt = (long)blockIdx.x * kThreads + threadIdx.x, nt = (long)gridDim.x * kThreads;
    for (long i = gt; i < a.B; i += nt) { a.last[i] = 0u; a.converged[i] = 1; }
    for (long i = gt; i < (long)a.B * a.Ms; i += nt) a.pieces[i] = 0;
    const long N = (long)a.B * a.H * a.W;
    for (long n = gt; n < N; n += nt) {
        const int l = a.labels[n];
        const bool mk = a.distance ? a.distance[n] >= a.d2 : a.markers[n] != 0;
        a.code[n] = (l > 0 && mk) ? (long long)l : 0ll;
    }
}

__global__ __launch_bounds__(kThreads) void split_tile_kernel(MarkArgs a) {
    __shared__ long long cls[kTile];
    __shared__ int lab[kTile];
    cc_tile_label(a, cls, lab);
}
__global__ __launch_bounds__(kThreads) void split_seam_kernel(MarkArgs a) { cc_seam_merge(a); }
// in place: words[n] parent -> root (cc_common.hpp, cc_flatten_area, on why that is sound)
__global__ __launch_bounds__(kThreads) void split_flatten_kernel(int* words, int* area, long HW, long N) {
    cc_flatten_area(words, words, area, HW, N, NoMark());
}

__global__ __launch_bounds__(kThreads) void split_init_kernel(SplitArgs a) {
    const long HW = (long)a.H * a.W, N = (long)a.B * HW;
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < N; n += (long)gridDim.x * kThreads) {
        const int r = a.root[n];                // -1 where the pixel is no marker pixel
        int o = 0;
        if (r >= 0 && a.area[(n / HW) * HW + r] >= a.min_marker_area) o = r + 1;
        a.dst[n] = o;
    }
}

// the smallest non-zero owner: owners travel as owner - 1 in unsigned, so that "none" (0) is the largest value
__device__ __forceinline__ unsigned take(unsigned best, int lab, int nl, int no) {
    const unsigned v = (unsigned)no - 1u;
    return (nl == lab && v < best) ? v : best;
}

__global__ __launch_bounds__(kThreads) void split_grow_kernel(SplitArgs a) {
    extern __shared__ int lds[];
    long blk = blockIdx.x;
    const int tx = (int)(blk % a.ntx); blk /= a.ntx;
    const int by = (int)(blk % a.nby);
    const int b = (int)(blk / a.nby);
    if (a.last[b] < (unsigned)a.launch) return;         // (workgroup-uniform) a fixed point: both planes hold it
    const int R = a.R, SW = a.SW, cells = R * SW;
    const int y0 = by * a.band - a.hy, x0 = tx * a.tw - a.hx;
    const long plane = (long)b * a.H * a.W;
    const int* lab_g = a.labels + plane;
    const int* src = a.src + plane;
    int* lab = lds;
    int* cur = lds + cells;
    int* nxt = lds + 2 * cells;
    for (int it = threadIdx.x; it < cells; it += kThreads) {
        const int ly = it / SW, lx = it - ly * SW, iy = y0 + ly, ix = x0 + lx;
        int l = 0, o = 0;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
            const long p = (long)iy * a.W + ix;
            l = lab_g[p];
            o = src[p];
        }
        lab[it] = l > 0 ? l : 0;
        cur[it] = o;
        nxt[it] = o;
    }
    __syncthreads();
    bool grew = false;                                  // this lane gave an OWNED cell an owner
    for (int s = 0; s < a.s_now; ++s) {
        // cells at least s from the staged edge hold this round's input; the round forms those at least s + 1 from it (along an
        // axis without a halo the staged edge is the image's: nothing lies beyond it)
        const int ylo = a.hy ? s + 1 : 0, yhi = R - ylo, xlo = a.hx ? s + 1 : 0, xhi = SW - xlo;
        const int rw = xhi - xlo, total = (yhi - ylo) * rw;
        bool any = false;
        for (int it = threadIdx.x; it < total; it += kThreads) {
            const int ly = ylo + it / rw, lx = xlo + it % rw, c = ly * SW + lx;
            const int l = lab[c];
            int o = cur[c];
            if (l > 0 && o == 0) {
                const bool up = ly > 0, dn = ly + 1 < R, lf = lx > 0, rt = lx + 1 < SW;
                unsigned best = 0xffffffffu;
                if (up) best = take(best, l, lab[c - SW], cur[c - SW]);
                if (dn) best = take(best, l, lab[c + SW], cur[c + SW]);
                if (lf) best = take(best, l, lab[c - 1], cur[c - 1]);
                if (rt) best = take(best, l, lab[c + 1], cur[c + 1]);
                if (a.conn8) {
                    if (up && lf) best = take(best, l, lab[c - SW - 1], cur[c - SW - 1]);
                    if (up && rt) best = take(best, l, lab[c - SW + 1], cur[c - SW + 1]);
                    if (dn && lf) best = take(best, l, lab[c + SW - 1], cur[c + SW - 1]);
                    if (dn && rt) best = take(best, l, lab[c + SW + 1], cur[c + SW + 1]);
                }
                if (best != 0xffffffffu) {
                    o = (int)(best + 1u);
                    any = true;
                    if (ly >= a.hy && ly < a.hy + a.band && lx >= a.hx && lx < a.hx + a.tw) grew = true;
                }
            }
            nxt[c] = o;
        }
        const int moved = __syncthreads_or(any ? 1 : 0);
        int* t = cur; cur = nxt; nxt = t;
        if (!moved) break;                              // (workgroup-uniform) cur == nxt on every cell a later round forms
    }
    int* dst = a.dst + plane;
    for (int it = threadIdx.x; it < a.band * a.tw; it += kThreads) {
        const int ly = a.hy + it / a.tw, lx = a.hx + it % a.tw, iy = y0 + ly, ix = x0 + lx;
        if (iy < a.H && ix < a.W) dst[(long)iy * a.W + ix] = cur[ly * SW + lx];        // (iy >= 0 and ix >= 0 for what a tile owns)
    }
    if (__ballot(grew) != 0ull && (threadIdx.x & 63) == 0) a.last[b] = (unsigned)a.launch + 1u;
}

__global__ __launch_bounds__(kThreads) void split_check_kernel(SplitArgs a) {
    const long HW = (long)a.H * a.W, N = (long)a.B * HW;
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < N; n += (long)gridDim.x * kThreads) {
        const int l = a.labels[n];
        if (l <= 0 || a.src[n] != 0) continue;
        const long b = n / HW, i = n - b * HW;
        const int y = (int)(i / a.W), x = (int)(i - (long)y * a.W);
        bool open = false;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if ((dy == 0 && dx == 0) || (!a.conn8 && dy != 0 && dx != 0)) continue;
                const int ny = y + dy, nx = x + dx;
                if (ny < 0 || ny >= a.H || nx < 0 || nx >= a.W) continue;
                const long m = b * HW + (long)ny * a.W + nx;
                open = open || (a.labels[m] == l && a.src[m] != 0);
            }
        if (open) a.converged[b] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void split_code_kernel(SplitArgs a) {
    const long N = (long)a.B * a.H * a.W;
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < N; n += (long)gridDim.x * kThreads) {
        const int l = a.labels[n];
        a.code[n] = l > 0 ? (((long long)l << 32) | (long long)(unsigned)a.src[n]) : 0ll;
    }
}

__global__ __launch_bounds__(kThreads) void split_fixup_kernel(SplitArgs a) {
    const long rows = (long)a.B * a.M;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < rows; i += (long)gridDim.x * kThreads) {
        const long b = i / a.M;
        const int k = (int)(i - b * a.M);
        int src = 0;
        if (k < a.count[b]) {                           // (rows from count[b] on are zero)
            long long* row = a.table + i * 9;
            src = (int)(row[0] >> 32);
            long long cls = -1;
            if (src >= 1 && src <= a.Ms) {
                cls = a.source_table[(b * a.Ms + (src - 1)) * 9];
                atomicAdd(a.pieces + b * a.Ms + (src - 1), 1);
            }
            row[0] = cls;
        }
        a.parent[i] = src;
    }
}

struct Plan { int band, tw, hy, hx, nby, ntx; };

// The tiling of an H x W image for launches of S rounds; rows / cols > 0: that band height / tile width.
//   tile width   kDefaultCols columns or the whole row where it is shorter
//   band height  kDefaultCols rows or the whole image where it is lower, evened out over the bands
// A halo of S cells lies on every side along which the image has more than one tile; the staged tile fits kLdsCells.
int make_plan(int H, int W, int S, int rows, int cols, Plan& p) {
    int tw = cols > 0 ? cols : kDefaultCols;
    if (tw > W) tw = W;
    int band = rows > 0 ? rows : kDefaultCols;
    if (band > H) band = H;
    if (rows <= 0) {
        const int nb = (H + band - 1) / band;
        band = (H + nb - 1) / nb;
    }
    p.band = band; p.tw = tw;
    p.nby = (H + band - 1) / band; p.ntx = (W + tw - 1) / tw;
    p.hy = p.nby > 1 ? S : 0; p.hx = p.ntx > 1 ? S : 0;
    if ((long)(band + 2 * p.hy) * (tw + 2 * p.hx) > kLdsCells) return UAPS_ERANGE;
    return UAPS_OK;
}

inline int check_dims(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if (H > kMaxExtent || W > kMaxExtent || (double)B * H * W * 8.0 >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}
// the code map, the labelling's workspace (which the marker pass uses first), two owner planes and the per-image words
inline double workspace_size(int B, int H, int W) { return (double)B * H * W * 24.0 + 4.0 * B * ((double)H * W / 256.0 + 2.0) + 6 * 256.0; }
inline size_t workspace_for(int B, int H, int W) {
    const size_t N = (size_t)B * H * W;
    return align256(8 * N) + align256(uaps::label_workspace_bytes(B, H, W)) + 2 * align256(4 * N) + align256(4 * (size_t)B);
}
inline bool sub_iters_ok(int S) { return S >= 0 && S <= kMaxS; }
}  // namespace

extern "C" int uaps_split_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    const int rc = check_dims(B, H, W);
    if (rc) return rc;
    if (workspace_size(B, H, W) >= kTooBig) return UAPS_ERANGE;
    *bytes = workspace_for(B, H, W);
    return UAPS_OK;
}

extern "C" int uaps_split_band_rows(int H, int W, int S, int* rows, int* cols) {
    if (!rows || !cols || H <= 0 || W <= 0 || !sub_iters_ok(S)) return UAPS_EINVAL;
    if (H > kMaxExtent || W > kMaxExtent) return UAPS_ERANGE;
    Plan p;
    const int rc = make_plan(H, W, S ? S : kDefaultS, 0, 0, p);
    if (rc) return rc;
    *rows = p.band; *cols = p.tw;
    return UAPS_OK;
}

extern "C" int uaps_split_instances(const uaps_split_call* call) {
    uaps_split_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.source_labels || !c.source_table || !c.labels || !c.count || !c.table || !c.parent || !c.pieces || !c.converged || !c.workspace)
        return UAPS_EINVAL;
    if ((c.distance != nullptr) == (c.markers != nullptr)) return UAPS_EINVAL;
    if (c.map1 && !c.map0) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0) return UAPS_EINVAL;
    if ((c.connectivity != 4 && c.connectivity != 8) || c.min_area < 1 || c.min_marker_area < 1) return UAPS_EINVAL;
    if (c.max_instances < 1 || c.source_rows < 1 || c.d2 < 0) return UAPS_EINVAL;
    if (c.max_iters < 1 || c.max_iters > UAPS_SPLIT_MAX_ITERS) return UAPS_EINVAL;
    if (!sub_iters_ok(c.sub_iters) || c.band_rows < 0 || c.tile_cols < 0) return UAPS_EINVAL;
    int rc = check_dims(c.B, c.H, c.W);
    if (rc) return rc;
    if ((double)c.B * c.max_instances * 72.0 >= kTooBig || (double)c.B * c.source_rows * 72.0 >= kTooBig) return UAPS_ERANGE;
    if (workspace_size(c.B, c.H, c.W) >= kTooBig) return UAPS_ERANGE;
    const int S = c.sub_iters ? c.sub_iters : kDefaultS;
    Plan p;
    rc = make_plan(c.H, c.W, S, c.band_rows, c.tile_cols, p);
    if (rc) return rc;
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, workspace_for(c.B, c.H, c.W))) return UAPS_EWORKSPACE;

    const long HW = (long)c.H * c.W, N = (long)c.B * HW;
    const size_t label_bytes = align256(uaps::label_workspace_bytes(c.B, c.H, c.W));
    char* ws = static_cast<char*>(c.workspace);
    long long* code = reinterpret_cast<long long*>(ws);
    char* label_ws = ws + align256(8 * (size_t)N);
    int* root = reinterpret_cast<int*>(label_ws);                                   // (the labelling's parent and area words come first)
    int* area = reinterpret_cast<int*>(label_ws + align256(4 * (size_t)N));
    int* own[2] = {reinterpret_cast<int*>(label_ws + label_bytes), reinterpret_cast<int*>(label_ws + label_bytes + align256(4 * (size_t)N))};
    hipStream_t st = (hipStream_t)c.stream;
    const dim3 block(kThreads), pix(grid_for(N, kMaxGrid));
    const int launches = (c.max_iters + S - 1) / S;
    uaps::account_bytes((double)N * (4.0 + (c.distance ? 4.0 : 1.0)));            // (the labelling accounts for its own operands)

    SplitArgs a;
    memset(&a, 0, sizeof a);
    a.B = c.B; a.H = c.H; a.W = c.W; a.conn8 = c.connectivity == 8 ? 1 : 0;
    a.d2 = c.d2; a.min_marker_area = c.min_marker_area; a.M = c.max_instances; a.Ms = c.source_rows;
    a.S = S; a.band = p.band; a.tw = p.tw; a.hy = p.hy; a.hx = p.hx; a.R = p.band + 2 * p.hy; a.SW = p.tw + 2 * p.hx;
    a.nby = p.nby; a.ntx = p.ntx;
    a.labels = c.source_labels; a.distance = c.distance; a.markers = c.markers; a.code = code; a.root = root; a.area = area;
    a.last = reinterpret_cast<unsigned*>(label_ws + label_bytes + 2 * align256(4 * (size_t)N));
    a.converged = c.converged; a.source_table = reinterpret_cast<const long long*>(c.source_table);
    a.table = reinterpret_cast<long long*>(c.table); a.count = c.count; a.parent = c.parent; a.pieces = c.pieces;
    hipLaunchKernelGGL(split_classify_kernel, pix, block, 0, st, a);

    MarkArgs m;
    memset(&m, 0, sizeof m);
    m.Q = c.B; m.H = c.H; m.W = c.W; m.ntx = (c.W + kTW - 1) / kTW; m.nty = (c.H + kTH - 1) / kTH;
    m.conn8 = a.conn8; m.mask = code; m.parent = root; m.area = area; m.pol.has_bg = 1; m.pol.bg = 0;
    const long tiles = (long)c.B * m.ntx * m.nty;               // < 2^28: every tile holds a pixel
    const long seam = (long)c.B * ((long)(m.nty - 1) * c.W + (long)(m.ntx - 1) * c.H);
    hipLaunchKernelGGL(split_tile_kernel, dim3((unsigned)tiles), block, 0, st, m);
    if (seam > 0) hipLaunchKernelGGL(split_seam_kernel, dim3(grid_for(seam, 1 << 24)), block, 0, st, m);
    hipLaunchKernelGGL(split_flatten_kernel, dim3(span_grid(N)), block, 0, st, root, area, HW, N);

    a.dst = own[0];
    hipLaunchKernelGGL(split_init_kernel, pix, block, 0, st, a);
    const size_t lds_bytes = (size_t)3 * a.R * a.SW * 4;                            // <= 64 KiB by make_plan
    const long blocks = (long)c.B * a.nby * a.ntx;                                  // <= B * H * W < 2^28
    for (int L = 0; L < launches; ++L) {
        a.launch = L;
        a.s_now = c.max_iters - L * S < S ? c.max_iters - L * S : S;
        a.src = own[L & 1]; a.dst = own[(L + 1) & 1];
        if (L == 0) UAPS_LAUNCH_MAIN(split_grow_kernel, dim3((unsigned)blocks), block, lds_bytes, st, a);
        else hipLaunchKernelGGL(split_grow_kernel, dim3((unsigned)blocks), block, lds_bytes, st, a);
    }
    a.src = own[launches & 1]; a.dst = nullptr;
    hipLaunchKernelGGL(split_check_kernel, pix, block, 0, st, a);
    hipLaunchKernelGGL(split_code_kernel, pix, block, 0, st, a);

    uaps_instances_call lc;
    memset(&lc, 0, sizeof lc);
    lc.struct_size = sizeof lc;
    lc.B = c.B; lc.H = c.H; lc.W = c.W; lc.connectivity = c.connectivity; lc.has_background = 1; lc.background = 0;
    lc.min_area = c.min_area; lc.max_instances = c.max_instances;
    lc.mask = reinterpret_cast<const int64_t*>(code); lc.map0 = c.map0; lc.map1 = c.map1;
    lc.labels = c.labels; lc.count = c.count; lc.table = c.table;
    lc.workspace = label_ws; lc.workspace_bytes = label_bytes; lc.stream = c.stream;
    rc = uaps::label_launches(lc);
    if (rc) return rc;
    hipLaunchKernelGGL(split_fixup_kernel, dim3(grid_for((long)c.B * c.max_instances, kMaxGrid)), block, 0, st, a);
    return (int)hipGetLastError();
}
