// Polygon rasterisation for gfx950 (include/uaps_hip.h, uaps_raster_plan / uaps_raster_fill): the exact even-odd fill of polygon rings
// into a label map -- the inverse of uaps_contours_trace / _write.  Ring points are integers in units of 2^-F pixel (F = frac_bits,
// s = 2^F), pixel (r, c) is sampled at its centre, and everything is int64 arithmetic in DOUBLED units: a row's centre is
// Yc = (2 r + 1) s; an edge A -> B crosses row r iff min(2 ya, 2 yb) <= Yc < max(2 ya, 2 yb); with (Y0, X0) the doubled endpoint of
// smaller Y, dy > 0 and dx the doubled differences to the other one and num = X0 dy + (Yc - Y0) dx, the first column at or right
// of the crossing is c0 = ceil((num - s dy) / (2 s dy)) clamped to [0, W].  Pixel (r, c) belongs to label k iff the number of
// crossings of k's edges in row r with c0 <= c is odd; a pixel takes the lowest label that owns it.
//
// Bit planes (morph.hip, skeleton.hip): every (image, label) owns one bit a pixel of its own clipped bounding box, rows x 64-bit
// words, so that overlapping labels never share a word.
//   plan   raster_zero_kernel, raster_extent_kernel: the box of every label's ring points -- integer atomicMax, the minima stored
//          inverted (hull.hip), one wave-combined set of atomics where a wave's points are of one label; every point learns its ring.
//          raster_scan_kernel: the words of every box scanned into its offset, the total for the host's one read.
//   fill   raster_clear_kernel: planes zero, the paint plane INT32_MAX, the sums zero.
//          raster_edges_kernel: a ring point owns the edge to its successor; every row the edge crosses toggles bit c0 of the box row
//          (64-bit atomic XOR).  An edge of more than `cut` rows is put on a list instead, and raster_long_kernel deals the list to
//          the waves of a fixed grid, an edge a wave, 64 rows a trip: the same toggles, and XOR does not care about their order.
//          raster_paint_kernel: a wave a word, a lane a bit.  The prefix XOR inside the word by shifts, the carry the parity of the
//          row's words before it; set pixels go to the paint plane by atomicMin (paint_pixel: a second owner leaves the lowest label
//          of the pixel less 2^30, so that the one plane also says "owned more than once"); the popcounts (area, and inter where
//          the reference label equals k) are summed in the wave over a run of words before one 64-bit atomic add.
//          raster_finish_kernel: the paint plane as int64 labels (and classes[label] as the mask), the pixels owned more than once
//          counted per image, one atomic a workgroup.
// Integers only, no float, no scratch; XOR / min / max / add atomics on integers, so two runs, both edge forms and any workspace
// contents give the same bits.
#include "call_common.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256; using uaps::u64;
typedef long long i64;

constexpr int kExtent = UAPS_RASTER_MAX_EXTENT, kMaxFrac = UAPS_RASTER_MAX_FRAC_BITS, kWaveRows = UAPS_RASTER_WAVE_ROWS;
constexpr int kFlatGrid = 2048, kPaintGrid = 4096, kLongGrid = 1024;
constexpr int kRun = 16;                                        // words a wave paints before it flushes its sums
constexpr int kNoLabel = 0x7fffffff;
constexpr int kTwice = 1 << 30;                                 // a pixel of more than one owner holds its lowest label less this
static_assert(kTooBig / 16.0 < (double)kTwice, "labels stay below 2^27: the sums' limit");
// doubled coordinates stay within 2^18, so num = X0 dy + (Yc - Y0) dx within 2^37 and 2 s dy within 2^23: far inside int64
static_assert(((i64)kExtent << kMaxFrac) * 2 <= 1LL << 18, "doubled coordinates within 2^18");
static_assert(kExtent <= 64 * 64, "a box row is at most 64 words: one lane a word for the carry");

struct RasterArgs {
    long N, L, E, HW;                   // points, rings, (image, label) pairs, pixels of an image
    int B, H, W, M, F, stride, cut;
    i64 background;
    const int* points;                  // [N][2], (y, x)
    const int* offsets;                 // [L + 1]
    const i64* rings;                   // [L][stride]: image, label, ...
    const int* reference;               // [B][H][W] or null
    const i64* classes;                 // [B][M] or null
    i64* totals;                        // the caller's [4]
    i64* head;                          // [0] words of all boxes  [1] boxes with a word  [2] box rows  [3] fill: edges on the list
    int* ext;                           // [E][4]: max y + 1, max (lim - y) + 1, max x + 1, max (lim - x) + 1; 0 = no point
    i64* woff;                          // [E + 1]: the first word of a box
    int* pring;                         // [N]: the ring of a point, -1 where it has no edge
    int* longs;                         // [N]: the points whose edge crosses more than `cut` rows, in no order
    int* paint;                         // [B][H][W]: the lowest label that owns a pixel, less kTwice where more than one does
    i64 n_words;                        // fill
    u64* planes;
    i64* labels;
    i64* mask;
    i64* stats;                         // [E][2]
    i64* overlap;                       // [B]
};

__device__ __forceinline__ i64 ceil_div(i64 a, i64 b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }      // b > 0
__device__ __forceinline__ int clampi(i64 v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }
__device__ __forceinline__ void add64(i64* p, i64 v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

// floor and ceiling of a / (2 s), s = 2^F, for |a| within 2^20
__device__ __forceinline__ int floor_2s(int a, int F) { return a >> (F + 1); }
__device__ __forceinline__ int ceil_2s(int a, int F) { return (a + (2 << F) - 1) >> (F + 1); }

// the clipped box of a label: rows r0 .. r0 + rows - 1, columns c0 .. c1, wpr words a row; rows == 0: no pixel centre can be inside
struct Box { int r0, rows, c0, c1, wpr; };
__device__ __forceinline__ Box box_of(const RasterArgs& A, long e) {
    Box b = {0, 0, 0, -1, 0};
    const int* x = A.ext + 4 * e;
    if (x[0] <= 0 || x[1] <= 0 || x[2] <= 0 || x[3] <= 0) return b;
    const int s = 1 << A.F, lim = kExtent << A.F;
    const int ymax = x[0] - 1, ymin = lim - (x[1] - 1), xmax = x[2] - 1, xmin = lim - (x[3] - 1);
    // a centre row lies in [2 ymin, 2 ymax); the first column right of a crossing at x is ceil((2 x - s) / (2 s)).  The divisor is
    // 2^(F + 1) and the values stay within 2^18: an arithmetic shift is the floor, and ceil(a / d) = floor((a + d - 1) / d)
    const int r0 = clampi(ceil_2s(2 * ymin - s, A.F), 0, A.H), r1 = clampi(floor_2s(2 * ymax - s - 1, A.F), -1, A.H - 1);
    const int c0 = clampi(ceil_2s(2 * xmin - s, A.F), 0, A.W), c1 = clampi(ceil_2s(2 * xmax - s, A.F), -1, A.W - 1);
    if (r1 < r0 || c1 < c0) return b;
    b.r0 = r0; b.rows = r1 - r0 + 1; b.c0 = c0; b.c1 = c1; b.wpr = (c1 - c0 + 64) >> 6;
    return b;
}

// the (image, label) pair of ring r, -1 for a ring outside the table
__device__ __forceinline__ long entry_of_ring(const RasterArgs& A, long r) {
    const i64 image = A.rings[r * A.stride], label = A.rings[r * A.stride + 1];
    if (image < 0 || image >= A.B || label < 1 || label > A.M) return -1;
    return (long)(image * A.M + (label - 1));
}

// ---- plan -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void raster_zero_kernel(RasterArgs A) {
    const long i0 = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i0 < 4) A.head[i0] = 0;
    for (long i = i0; i < 4 * A.E; i += (long)gridDim.x * kThreads) A.ext[i] = 0;
}

__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

__global__ __launch_bounds__(kThreads) void raster_extent_kernel(RasterArgs A) {
    const int lane = threadIdx.x & 63, lim = kExtent << A.F;
    for (long base = (long)blockIdx.x * kThreads; base < A.N; base += (long)gridDim.x * kThreads) {      // (the same trips in every lane)
        const long i = base + threadIdx.x;
        long e = -1;
        int v[4] = {0, 0, 0, 0};
        if (i < A.N) {
            long lo = 0, hi = A.L - 1;                                  // the last ring whose first point is at or before i
            while (lo < hi) {
                const long mid = (lo + hi + 1) >> 1;
                if (A.offsets[mid] <= i) lo = mid; else hi = mid - 1;
            }
            const long a = A.offsets[lo], b = A.offsets[lo + 1];
            const bool ok = a >= 0 && a <= i && i < b && b <= A.N && b - a >= 3;      // fewer than 3 points: nothing
            if (ok) e = entry_of_ring(A, lo);
            A.pring[i] = e >= 0 ? (int)lo : -1;
            if (e >= 0) {
                const int y = clampi(A.points[2 * i], 0, lim), x = clampi(A.points[2 * i + 1], 0, lim);
                v[0] = y + 1; v[1] = lim - y + 1; v[2] = x + 1; v[3] = lim - x + 1;
            }
        }
        const u64 live = __ballot(e >= 0);
        if (!live) continue;
        const long first = __shfl(e, __ffsll((long long)live) - 1, 64);
        if (__all(e < 0 || e == first)) {                               // one label in the wave: one set of atomics
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = wave_max_int(v[c]);
            if (lane < 4) atomicMax(A.ext + 4 * first + lane, lane == 0 ? v[0] : (lane == 1 ? v[1] : (lane == 2 ? v[2] : v[3])));
        } else if (e >= 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) atomicMax(A.ext + 4 * e + c, v[c]);
        }
    }
}

// exclusive prefix of v over the block; total: the block's sum, in every thread
__device__ __forceinline__ i64 block_scan(i64 v, i64* red, i64& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    i64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const i64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                    // (red may still be read from the scan before)
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    i64 base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) { base += w < wave ? red[w] : 0; total += red[w]; }
    return base + inc - v;
}

// one workgroup, a run of consecutive table rows a thread, one scan of the threads' sums: the table has B * max_instances rows, a few
// thousand
__global__ __launch_bounds__(kThreads) void raster_scan_kernel(RasterArgs A) {
    __shared__ i64 red[kWaves];
    const long per = (A.E + kThreads - 1) / kThreads;
    const long e0 = threadIdx.x * per, e1 = e0 + per < A.E ? e0 + per : A.E;
    i64 words = 0, boxes = 0, rows = 0;
    for (long e = e0; e < e1; ++e) {
        const Box b = box_of(A, e);
        words += (i64)b.rows * b.wpr; boxes += b.rows > 0; rows += b.rows;
    }
    i64 total, all_boxes, all_rows;
    i64 at = block_scan(words, red, total);
    block_scan(boxes, red, all_boxes);
    block_scan(rows, red, all_rows);
    for (long e = e0; e < e1; ++e) {
        const Box b = box_of(A, e);
        A.woff[e] = at;
        at += (i64)b.rows * b.wpr;
    }
    if (threadIdx.x == 0) {
        A.woff[A.E] = total;
        A.head[0] = total; A.head[1] = all_boxes; A.head[2] = all_rows; A.head[3] = 0;
        A.totals[0] = total; A.totals[1] = all_boxes; A.totals[2] = all_rows; A.totals[3] = 0;
    }
}

// ---- fill -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void raster_clear_kernel(RasterArgs A) {
    if (A.head[0] != A.n_words) return;                                 // not the workspace the caller read its total from
    const long i0 = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    for (long i = i0; i < A.n_words; i += step) A.planes[i] = 0ull;
    if (i0 == 0) A.head[3] = 0;
    for (long i = i0; i < A.B * A.HW; i += step) A.paint[i] = kNoLabel;
    for (long i = i0; i < 2 * A.E; i += step) A.stats[i] = 0;
    for (long i = i0; i < A.B; i += step) A.overlap[i] = 0;
}

// the edge from point i to its successor, in doubled units from its endpoint of smaller Y, and the box rows it crosses
struct Edge { i64 X0, Y0, dy, dx; int ra, rb, cfix; long base; Box box; };
__device__ __forceinline__ int column_of(const RasterArgs& A, const Edge& g, int r) {
    const i64 s = 1LL << A.F, Yc = (2LL * r + 1) * s;
    const i64 num = g.X0 * g.dy + (Yc - g.Y0) * g.dx;
    return clampi(ceil_div(num - s * g.dy, 2 * s * g.dy), 0, A.W);
}

__device__ __forceinline__ bool edge_of(const RasterArgs& A, long i, Edge& g) {
    const long r = A.pring[i];
    if (r < 0 || r >= A.L) return false;
    const long a = A.offsets[r], b = A.offsets[r + 1];
    if (a < 0 || i < a || i >= b || b > A.N) return false;
    const long e = entry_of_ring(A, r);
    if (e < 0) return false;
    const long j = i + 1 < b ? i + 1 : a;                               // the last edge closes the ring
    const int lim = kExtent << A.F;
    const i64 ya = 2 * clampi(A.points[2 * i], 0, lim), xa = 2 * clampi(A.points[2 * i + 1], 0, lim);
    const i64 yb = 2 * clampi(A.points[2 * j], 0, lim), xb = 2 * clampi(A.points[2 * j + 1], 0, lim);
    if (ya == yb) return false;                                         // horizontal edges never cross
    const bool up = ya < yb;
    g.Y0 = up ? ya : yb; g.X0 = up ? xa : xb;
    g.dy = up ? yb - ya : ya - yb; g.dx = up ? xb - xa : xa - xb;
    g.box = box_of(A, e);
    if (g.box.rows == 0) return false;
    const i64 s = 1LL << A.F;
    // Y0 <= (2 r + 1) s < Y0 + dy, inside the box (which holds every such row of the frame already)
    g.ra = clampi(ceil_2s((int)(g.Y0 - s), A.F), g.box.r0, A.H);
    g.rb = clampi(floor_2s((int)(g.Y0 + g.dy - s - 1), A.F), -1, g.box.r0 + g.box.rows - 1);
    if (g.rb < g.ra) return false;
    g.base = (long)A.woff[e];
    g.cfix = g.dx == 0 ? column_of(A, g, g.ra) : -1;                    // a vertical edge: one column for all its rows
    return true;
}

__device__ __forceinline__ void toggle(const RasterArgs& A, const Edge& g, int r) {
    const int c = g.cfix >= 0 ? g.cfix : column_of(A, g, r);
    if (c < g.box.c0 || c > g.box.c1) return;                           // (c0 = W toggles nothing)
    const int bit = c - g.box.c0;
    const long at = g.base + (long)(r - g.box.r0) * g.box.wpr + (bit >> 6);
    if (at >= 0 && at < A.n_words) atomicXor(A.planes + at, 1ull << (bit & 63));
}

__global__ __launch_bounds__(kThreads) void raster_edges_kernel(RasterArgs A) {
    if (A.head[0] != A.n_words) return;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < A.N; i += (long)gridDim.x * kThreads) {
        Edge g;
        if (!edge_of(A, i, g)) continue;
        if (g.rb - g.ra + 1 > A.cut) {                                  // a long edge: left to a wave of raster_long_kernel
            const u64 at = atomicAdd(reinterpret_cast<u64*>(A.head + 3), 1ull);
            if (at < (u64)A.N) A.longs[at] = (int)i;
            continue;
        }
        for (int r = g.ra; r <= g.rb; ++r) toggle(A, g, r);
    }
}

// the list of long edges over a fixed grid: an edge a wave, 64 rows a trip
__global__ __launch_bounds__(kThreads) void raster_long_kernel(RasterArgs A) {
    if (A.head[0] != A.n_words) return;
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * kWaves;
    i64 count = A.head[3];
    if (count > A.N) count = A.N;
    for (long j = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); j < count; j += waves) {
        const long k = A.longs[j];
        Edge w;
        if (k < 0 || k >= A.N || !edge_of(A, k, w)) continue;           // (the same in every lane)
        for (int r = w.ra + lane; r <= w.rb; r += 64) toggle(A, w, r);
    }
}

// A set pixel of label k on the paint plane.  The first owner leaves k; every later one sees that the pixel was owned and leaves the
// lower of k and the label it saw, less kTwice -- below every plain label.  Whatever the order, the plane ends at the lowest label
// of the pixel, less kTwice iff it has more than one owner: the lowest label either comes later than another owner and posts itself
// so, or comes first, and the owner next after it sees it and posts it.
__device__ __forceinline__ void paint_pixel(int* p, int k) {
    const int old = atomicMin(p, k);
    if (old == kNoLabel) return;
    const int low = old < 0 ? old + kTwice : old;
    atomicMin(p, (k < low ? k : low) - kTwice);
}

__global__ __launch_bounds__(kThreads) void raster_paint_kernel(RasterArgs A) {
    if (A.head[0] != A.n_words) return;
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * kWaves, runs = (A.n_words + kRun - 1) / kRun;
    for (long run = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); run < runs; run += waves) {
        const long w0 = run * kRun, w1 = w0 + kRun < A.n_words ? w0 + kRun : A.n_words;
        long lo = 0, hi = A.E - 1;                                      // the last box that starts at or before w0: it holds w0
        while (lo < hi) {
            const long mid = (lo + hi + 1) >> 1;
            if (A.woff[mid] <= w0) lo = mid; else hi = mid - 1;
        }
        long e = lo, first = A.woff[e], end = A.woff[e + 1];
        Box bx = box_of(A, e);
        i64 area = 0, inter = 0;
        for (long w = w0; w < w1; ++w) {
            while (w >= end && e + 1 < A.E) {                           // the next box with a word
                if (lane == 0 && area) { add64(A.stats + 2 * e, area); if (inter) add64(A.stats + 2 * e + 1, inter); }
                area = inter = 0;
                ++e; first = end; end = A.woff[e + 1];
                bx = box_of(A, e);
            }
            if (bx.wpr < 1 || w < first || w >= end) break;             // (a workspace that is not the plan's)
            const long local = w - first;
            const int row = (int)(local / bx.wpr), wi = (int)(local % bx.wpr);
            u64 f = A.planes[w];
            const int odd = lane < wi ? __popcll(A.planes[w - wi + lane]) & 1 : 0;      // the row's words before this one
            const bool carry = __popcll(__ballot(odd)) & 1;
            f ^= f << 1; f ^= f << 2; f ^= f << 4; f ^= f << 8; f ^= f << 16; f ^= f << 32;      // bit j: the parity of bits 0 .. j
            if (carry) f = ~f;
            const int col = bx.c0 + 64 * wi + lane, r = bx.r0 + row;
            const bool set = col <= bx.c1 && r < A.H && ((f >> lane) & 1ull);
            const int k = (int)(e % A.M) + 1;
            const long pix = (e / A.M) * A.HW + (long)r * A.W + col;
            bool hit = false;
            if (set) {
                paint_pixel(A.paint + pix, k);
                hit = A.reference && A.reference[pix] == k;
            }
            area += __popcll(__ballot(set));
            inter += __popcll(__ballot(hit));
        }
        if (lane == 0 && area) { add64(A.stats + 2 * e, area); if (inter) add64(A.stats + 2 * e + 1, inter); }
    }
}

// blockIdx.y strides over the images
__global__ __launch_bounds__(kThreads) void raster_finish_kernel(RasterArgs A) {
    if (A.head[0] != A.n_words) return;
    __shared__ int red[kWaves];
    for (long b = blockIdx.y; b < A.B; b += gridDim.y) {
        int twice = 0;
        for (long p = (long)blockIdx.x * kThreads + threadIdx.x; p < A.HW; p += (long)gridDim.x * kThreads) {
            const long at = b * A.HW + p;
            const int raw = A.paint[at], v = raw < 0 ? raw + kTwice : raw;
            const bool owned = v >= 1 && v <= A.M;
            A.labels[at] = owned ? (i64)v : A.background;
            if (A.mask) A.mask[at] = owned ? A.classes[b * A.M + (v - 1)] : 0;
            twice += owned && raw < 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) twice += __shfl_xor(twice, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = twice;
        __syncthreads();
        if (threadIdx.x == 0) {
            i64 sum = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) sum += red[w];
            if (sum) add64(A.overlap + b, sum);
        }
        __syncthreads();
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
struct Layout { size_t head, ext, woff, pring, longs, paint, bytes; };

int lay_out(i64 n_points, i64 n_rings, int B, int H, int W, int M, Layout& L) {
    if (n_points < 1 || n_rings < 1 || B < 1 || H < 1 || W < 1 || M < 1) return UAPS_EINVAL;
    if (H > kExtent || W > kExtent) return UAPS_ERANGE;
    if (n_points >= 1073741824LL || n_rings >= 1073741824LL) return UAPS_ERANGE;      // (2 * n_points indexes the coordinates)
    if ((double)B * H * W * 8.0 >= kTooBig || (double)B * M * 16.0 >= kTooBig) return UAPS_ERANGE;      // labels; the boxes and the sums
    const size_t N = (size_t)n_points, E = (size_t)B * M, P = (size_t)B * H * W;
    size_t o = 0;
    L.head = o; o += 256;
    L.ext = o; o = align256(o + E * 16);
    L.woff = o; o = align256(o + (E + 1) * 8);
    L.pring = o; o = align256(o + N * 4);
    L.longs = o; o = align256(o + N * 4);
    L.paint = o; o = align256(o + P * 4);
    L.bytes = o;
    return UAPS_OK;
}

// the checks both entry points share, and the kernels' arguments
int prepare(const uaps_raster_call* call, uaps_raster_call& c, RasterArgs& a) {
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.points || !c.ring_offsets || !c.rings || !c.workspace) return UAPS_EINVAL;
    if ((const void*)c.points == (const void*)c.ring_offsets || (const void*)c.points == (const void*)c.rings ||
        (const void*)c.ring_offsets == (const void*)c.rings) return UAPS_EINVAL;
    if (c.frac_bits < 0 || c.frac_bits > kMaxFrac || c.ring_stride < 2 || c.ring_stride > 64) return UAPS_EINVAL;
    if (c.edge_wave_rows < UAPS_RASTER_ALL_WAVE || c.edge_wave_rows > kExtent) return UAPS_EINVAL;
    Layout L;
    const int rc = lay_out(c.n_points, c.n_rings, c.B, c.H, c.W, c.max_instances, L);
    if (rc) return rc;
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, L.bytes)) return UAPS_EWORKSPACE;
    memset(&a, 0, sizeof a);
    char* ws = reinterpret_cast<char*>(c.workspace);
    a.N = (long)c.n_points; a.L = (long)c.n_rings; a.E = (long)c.B * c.max_instances; a.HW = (long)c.H * c.W;
    a.B = c.B; a.H = c.H; a.W = c.W; a.M = c.max_instances; a.F = c.frac_bits; a.stride = c.ring_stride;
    a.cut = c.edge_wave_rows == 0 ? kWaveRows : (c.edge_wave_rows == UAPS_RASTER_ALL_WAVE ? 0 : c.edge_wave_rows);
    a.points = c.points; a.offsets = c.ring_offsets; a.rings = reinterpret_cast<const i64*>(c.rings);
    a.head = reinterpret_cast<i64*>(ws + L.head);
    a.ext = reinterpret_cast<int*>(ws + L.ext);
    a.woff = reinterpret_cast<i64*>(ws + L.woff);
    a.pring = reinterpret_cast<int*>(ws + L.pring);
    a.longs = reinterpret_cast<int*>(ws + L.longs);
    a.paint = reinterpret_cast<int*>(ws + L.paint);
    return UAPS_OK;
}
}  // namespace

extern "C" int uaps_raster_workspace_bytes(int64_t n_points, int64_t n_rings, int B, int H, int W, int max_instances, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    Layout L;
    const int rc = lay_out(n_points, n_rings, B, H, W, max_instances, L);
    if (rc) return rc;
    *bytes = L.bytes;
    return UAPS_OK;
}

extern "C" int uaps_raster_plan(const uaps_raster_call* call) {
    uaps_raster_call c;
    RasterArgs a;
    const int rc = prepare(call, c, a);
    if (rc) return rc;
    if (!c.totals || (const void*)c.totals == (const void*)c.points || (const void*)c.totals == (const void*)c.ring_offsets ||
        (const void*)c.totals == (const void*)c.rings) return UAPS_EINVAL;
    a.totals = reinterpret_cast<i64*>(c.totals);
    hipStream_t st = (hipStream_t)c.stream;
    uaps::account_bytes(8.0 * (double)a.N + 4.0 * (double)(a.L + 1) + 16.0 * (double)a.L + 4.0 * (double)a.N + 24.0 * (double)a.E);
    const dim3 block(kThreads);
    hipLaunchKernelGGL(raster_zero_kernel, dim3(grid_for(4 * a.E, kFlatGrid)), block, 0, st, a);
    UAPS_LAUNCH_MAIN(raster_extent_kernel, dim3(grid_for(a.N, kFlatGrid)), block, 0, st, a);
    hipLaunchKernelGGL(raster_scan_kernel, dim3(1), block, 0, st, a);
    return (int)hipGetLastError();
}

extern "C" int uaps_raster_fill(const uaps_raster_call* call) {
    uaps_raster_call c;
    RasterArgs a;
    const int rc = prepare(call, c, a);
    if (rc) return rc;
    if (!c.planes || !c.labels || !c.stats || !c.overlap || (c.classes == nullptr) != (c.mask == nullptr)) return UAPS_EINVAL;
    const void* p[] = {c.points, c.ring_offsets, c.rings, c.reference, c.classes, c.planes, c.labels, c.mask, c.stats, c.overlap};
    for (int i = 0; i < 10; ++i)
        for (int j = (i < 5 ? 5 : i + 1); j < 10; ++j)                  // an output equal to an input or to another output
            if (p[i] && p[i] == p[j]) return UAPS_EINVAL;
    if (c.n_words < 1) return UAPS_EINVAL;
    if ((double)c.n_words * 8.0 >= kTooBig) return UAPS_ERANGE;
    a.n_words = c.n_words; a.planes = reinterpret_cast<u64*>(c.planes);
    a.reference = c.reference; a.classes = reinterpret_cast<const i64*>(c.classes); a.background = c.background;
    a.labels = reinterpret_cast<i64*>(c.labels); a.mask = reinterpret_cast<i64*>(c.mask);
    a.stats = reinterpret_cast<i64*>(c.stats); a.overlap = reinterpret_cast<i64*>(c.overlap);
    hipStream_t st = (hipStream_t)c.stream;
    const double pixels = (double)a.B * (double)a.HW;
    uaps::account_bytes(16.0 * (double)a.N + 24.0 * (double)a.n_words + (12.0 + 8.0 + (c.reference ? 4.0 : 0.0) + (c.mask ? 8.0 : 0.0) + 8.0) * pixels);
    const dim3 block(kThreads);
    const long most = a.n_words > a.B * a.HW ? a.n_words : a.B * a.HW;
    const long runs = (a.n_words + kRun - 1) / kRun;
    hipLaunchKernelGGL(raster_clear_kernel, dim3(grid_for(most, kFlatGrid)), block, 0, st, a);
    hipLaunchKernelGGL(raster_edges_kernel, dim3(grid_for(a.N, kFlatGrid)), block, 0, st, a);
    if (a.cut < kExtent)                                                // (no edge crosses more than kExtent rows)
        hipLaunchKernelGGL(raster_long_kernel, dim3((int)((a.N + kWaves - 1) / kWaves < kLongGrid ? (a.N + kWaves - 1) / kWaves : kLongGrid)), block, 0, st, a);
    UAPS_LAUNCH_MAIN(raster_paint_kernel, dim3((int)((runs + kWaves - 1) / kWaves < kPaintGrid ? (runs + kWaves - 1) / kWaves : kPaintGrid)), block, 0, st, a);
    hipLaunchKernelGGL(raster_finish_kernel, dim3(grid_for(a.HW, 256), a.B < 4096 ? a.B : 4096), block, 0, st, a);
    return (int)hipGetLastError();
}
