// Defect skeletons for gfx950 (include/uaps_hip.h): uaps_skeletonize, Guo and Hall's two-subiteration parallel thinning of the
// selected classes of an int64 label map on packed bit planes, and uaps_skeleton_stats, the per-defect link, end and branch counts of
// a skeleton.
//
// uaps_skeletonize
//   skel_pack_kernel     int64 map -> bit planes [class][B][H][nw] of 64-bit words in half 0 of the workspace: on wave64 a ballot of
//                        mask == c over 64 consecutive pixels IS the word (morph.hip's staging).  Tail bits of a row's last word are 0
//                        and stay 0 (thinning only removes).  Also resets the per-image words.
//   skel_thin_kernel     launch L reads half L % 2 and writes the other: S sub-iterations on a tile of `band` rows x `tw` words of ONE
//                        plane of one image, staged in LDS with S halo rows above and below and, where the image is wider than the
//                        tile, one halo word (64 >= S pixels) left and right.  A sub-iteration looks one pixel far, so after s of them
//                        the outer s pixels of the staged tile are stale and the owned pixels never are (morph.hip's reach argument);
//                        sub-iteration s therefore only forms rows [s + 1, R - s - 1).  Rows and words outside the image or outside
//                        the staged tile read as 0 at every read.
//   bit-sliced rule      the eight neighbour words of a word come from the three rows and one-bit shifts with carries from the adjacent
//                        words; "C = 1" and "N in {2, 3}" are boolean formulas on four one-bit terms each (exactly_one, at_least_two,
//                        all_four below): no per-pixel branch, no table.
//   convergence          last[b] = 1 + the index of the last launch that removed a pixel from an owned word of image b (a plain store
//                        of that constant).  Launch L returns at once where last[b] < L: launch L - 1 made S / 2 >= 1 whole iterations
//                        and removed nothing, so the plane is a fixed point and BOTH halves already hold it.
//   skel_check_kernel    the returned planes are a fixed point iff neither sub-iteration's rule deletes anything from them (the second
//                        then sees the same plane as the first): one pass, one-pixel reach, clears converged[b] where something would go.
//   skel_unpack_kernel   planes + the input map -> the int64 result: a selected pixel whose bit is gone becomes the background.
// uaps_skeleton_stats
//   skeleton_stats_kernel<PLANE, LDS> is built like shapes.hip's shape_accumulate_kernel: a wave owns 64 consecutive pixels of a row,
//   reads rows y - 1, y, y + 1 and takes the side neighbours from shuffles; every link is counted by its raster-first end (E, SW, S,
//   SE); the five counts travel as one packed word (12 bits each: a group adds at most 128 to a field) and are reduced over runs of
//   equal labels (cc_common.hpp's run_end); the flush is table_flush.hpp's, shared with shapes.hip.
// Integers only, no float, no scratch, no host synchronisation.
#include "cc_common.hpp"
#include "table_flush.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256; using uaps::u64;
using uaps::cc::run_end;
using uaps::table::table_lds_zero;
using uaps::table::table_lds_flush;

constexpr int kMaxSel = UAPS_SKEL_MAX_CLASSES, kMaxExtent = UAPS_SKEL_MAX_EXTENT, kMaxS = UAPS_SKEL_MAX_SUB_ITERS;
constexpr int kLdsWords = 64 * 1024 / 8;        // the budget of a workgroup, in 64-bit words
constexpr int kMaxTileWords = 8;                // a tile is at most 512 pixels wide
constexpr int kDefaultS = 8;                    // sub-iterations a launch (the S sweep)
constexpr int kMaxGrid = 1 << 20;

// ---- the rule on words ----------------------------------------------------------------------------------------------------------
// of four one-bit terms a, b, c, d, per bit
__device__ __forceinline__ u64 exactly_one(u64 a, u64 b, u64 c, u64 d) { return ((a ^ b) ^ (c ^ d)) & ~((a & b) | (c & d)); }
__device__ __forceinline__ u64 at_least_two(u64 a, u64 b, u64 c, u64 d) { return (a & b) | (c & d) | ((a ^ b) & (c ^ d)); }
__device__ __forceinline__ u64 all_four(u64 a, u64 b, u64 c, u64 d) { return a & b & c & d; }

// The neighbour words of the word m (rows above, of, below it: u*, m*, d*; *p / *n the words left / right of it).  Bit i of a word
// is column 64 j + i: the EAST neighbour of bit i is bit i + 1.
struct Nbrs { u64 p2, p3, p4, p5, p6, p7, p8, p9; };
__device__ __forceinline__ u64 east(u64 c, u64 n) { return (c >> 1) | (n << 63); }
__device__ __forceinline__ u64 west(u64 p, u64 c) { return (c << 1) | (p >> 63); }
__device__ __forceinline__ Nbrs neighbours(u64 up, u64 uc, u64 un, u64 mp, u64 mc, u64 mn, u64 dp, u64 dc, u64 dn) {
    Nbrs n;
    n.p2 = uc; n.p3 = east(uc, un); n.p4 = east(mc, mn); n.p5 = east(dc, dn);
    n.p6 = dc; n.p7 = west(dp, dc); n.p8 = west(mp, mc); n.p9 = west(up, uc);
    return n;
}
// the pixels of m that satisfy C = 1 and 2 <= min(N1, N2) <= 3
__device__ __forceinline__ u64 simple_pixels(u64 m, const Nbrs& n) {
    const u64 a1 = n.p9 | n.p2, a2 = n.p3 | n.p4, a3 = n.p5 | n.p6, a4 = n.p7 | n.p8;       // N1's terms
    const u64 b1 = n.p2 | n.p3, b2 = n.p4 | n.p5, b3 = n.p6 | n.p7, b4 = n.p8 | n.p9;       // N2's terms
    const u64 c1 = ~n.p2 & a2, c2 = ~n.p4 & a3, c3 = ~n.p6 & a4, c4 = ~n.p8 & a1;           // C's terms
    return m & exactly_one(c1, c2, c3, c4) & at_least_two(a1, a2, a3, a4) & at_least_two(b1, b2, b3, b4) &
           ~(all_four(a1, a2, a3, a4) & all_four(b1, b2, b3, b4));
}
__device__ __forceinline__ u64 deleted_first(u64 m, const Nbrs& n) { return simple_pixels(m, n) & ~((n.p2 | n.p3 | ~n.p5) & n.p4); }
__device__ __forceinline__ u64 deleted_second(u64 m, const Nbrs& n) { return simple_pixels(m, n) & ~((n.p6 | n.p7 | ~n.p9) & n.p8); }

// ---- uaps_skeletonize -------------------------------------------------------------------------------------------------------------
struct SkelArgs {
    int B, H, W, nw;            // nw: words of a row
    int n;                      // selected classes
    int S, s_now, launch;       // halo rows, sub-iterations of this launch, its index
    int band, R;                // owned rows, staged rows = band + 2 S
    int tw, sw, hx, ntx, nby;   // owned words, staged words = tw + 2 hx, halo words per side (0 | 1), tiles per row, bands per image
    long long cls[kMaxSel], bg;
    const long long* mask;
    long long* out;
    const u64* src;             // [n][B][H][nw]
    u64* dst;
    unsigned* last;             // [B]
    unsigned char* converged;   // [B]
};

__global__ __launch_bounds__(kThreads) void skel_pack_kernel(SkelArgs a) {
    const int lane = threadIdx.x & 63;
    const long gt = (long)blockIdx.x * kThreads + threadIdx.x, nt = (long)gridDim.x * kThreads;
    for (long i = gt; i < a.B; i += nt) { a.last[i] = 0u; a.converged[i] = 1; }
    long long cls[kMaxSel];
#pragma unroll
    for (int k = 0; k < kMaxSel; ++k) cls[k] = a.cls[k];
    const long words = (long)a.B * a.H * a.nw;          // of one plane
    for (long w = gt >> 6; w < words; w += nt >> 6) {   // (wave-uniform)
        const int j = (int)(w % a.nw);
        const long row = w / a.nw;                      // b * H + y
        const int x = j * 64 + lane;
        const bool in = x < a.W;
        long long v = a.bg;
        if (in) v = a.mask[row * a.W + x];
#pragma unroll
        for (int k = 0; k < kMaxSel; ++k) {
            if (k >= a.n) break;
            const u64 word = __ballot(in && v == cls[k]);
            if (lane == k) a.dst[(long)k * words + w] = word;
        }
    }
}

__global__ __launch_bounds__(kThreads) void skel_thin_kernel(SkelArgs a) {
    extern __shared__ u64 lds[];
    long blk = blockIdx.x;
    const int tx = (int)(blk % a.ntx); blk /= a.ntx;
    const int by = (int)(blk % a.nby); blk /= a.nby;
    const int b = (int)(blk % a.B), k = (int)(blk / a.B);
    if (a.last[b] < (unsigned)a.launch) return;         // (workgroup-uniform) converged: both halves hold the fixed point
    const int R = a.R, sw = a.sw, ps = R * sw;
    const int ry0 = by * a.band - a.S, gj0 = tx * a.tw - a.hx;
    const long plane = ((long)k * a.B + b) * a.H * a.nw;
    const u64* src = a.src + plane;
    u64* cur = lds;
    u64* nxt = lds + ps;
    for (int it = threadIdx.x; it < ps; it += kThreads) {
        const int lr = it / sw, lj = it - lr * sw, iy = ry0 + lr, gj = gj0 + lj;
        u64 v = 0ull;
        if (iy >= 0 && iy < a.H && gj >= 0 && gj < a.nw) v = src[(long)iy * a.nw + gj];
        cur[it] = v;
    }
    __syncthreads();
    u64 gone = 0ull;                                    // what this lane removed from owned words
    for (int s = 0; s < a.s_now; ++s) {
        const int lo = s + 1, hi = R - s - 1;           // rows [s, R - s) hold this sub-iteration's input
        const int total = (hi - lo) * sw;
        for (int it = threadIdx.x; it < total; it += kThreads) {
            const int lr = lo + it / sw, lj = it % sw;
            const bool hp = lj > 0, hn = lj + 1 < sw;   // a word outside the staged tile reads as 0
            const u64* m = cur + lr * sw + lj;
            const u64* u = m - sw;
            const u64* d = m + sw;
            const u64 mc = *m;
            const Nbrs nb = neighbours(hp ? u[-1] : 0ull, *u, hn ? u[1] : 0ull, hp ? m[-1] : 0ull, mc, hn ? m[1] : 0ull,
                                       hp ? d[-1] : 0ull, *d, hn ? d[1] : 0ull);
            const u64 del = (s & 1) ? deleted_second(mc, nb) : deleted_first(mc, nb);
            nxt[lr * sw + lj] = mc & ~del;
            if (lr >= a.S && lr < a.S + a.band && lj >= a.hx && lj < a.hx + a.tw) gone |= del;
        }
        __syncthreads();
        u64* t = cur; cur = nxt; nxt = t;
    }
    u64* dst = a.dst + plane;
    for (int it = threadIdx.x; it < a.band * a.tw; it += kThreads) {
        const int lr = a.S + it / a.tw, lj = a.hx + it % a.tw, iy = ry0 + lr, gj = gj0 + lj;
        if (iy < a.H && gj < a.nw) dst[(long)iy * a.nw + gj] = cur[lr * sw + lj];       // (iy >= 0 and gj >= 0 for what a tile owns)
    }
    if (__ballot(gone != 0ull) != 0ull && (threadIdx.x & 63) == 0) a.last[b] = (unsigned)a.launch + 1u;
}

// one lane per word of a plane: would either sub-iteration delete anything from it?
__global__ __launch_bounds__(kThreads) void skel_check_kernel(SkelArgs a) {
    const long per = (long)a.H * a.nw, total = (long)a.n * a.B * per;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
        const long pl = i / per, rem = i - pl * per;
        const int y = (int)(rem / a.nw), j = (int)(rem - (long)y * a.nw);
        const u64* m = a.src + i;
        const u64 mc = *m;
        if (mc == 0ull) continue;
        const bool hu = y > 0, hd = y < a.H - 1, hp = j > 0, hn = j < a.nw - 1;
        const u64* u = m - a.nw;
        const u64* d = m + a.nw;
        const Nbrs nb = neighbours(hu && hp ? u[-1] : 0ull, hu ? *u : 0ull, hu && hn ? u[1] : 0ull, hp ? m[-1] : 0ull, mc,
                                   hn ? m[1] : 0ull, hd && hp ? d[-1] : 0ull, hd ? *d : 0ull, hd && hn ? d[1] : 0ull);
        if ((deleted_first(mc, nb) | deleted_second(mc, nb)) != 0ull) a.converged[pl % a.B] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void skel_unpack_kernel(SkelArgs a) {
    const int lane = threadIdx.x & 63;
    const long gt = (long)blockIdx.x * kThreads + threadIdx.x, nt = (long)gridDim.x * kThreads;
    long long cls[kMaxSel];
#pragma unroll
    for (int k = 0; k < kMaxSel; ++k) cls[k] = a.cls[k];
    const long words = (long)a.B * a.H * a.nw;
    for (long w = gt >> 6; w < words; w += nt >> 6) {   // (wave-uniform)
        const int j = (int)(w % a.nw);
        const long row = w / a.nw;
        const int x = j * 64 + lane;
        if (x >= a.W) continue;
        const long px = row * a.W + x;
        long long v = a.mask[px];
#pragma unroll
        for (int k = 0; k < kMaxSel; ++k) {
            if (k >= a.n) break;
            if (v == cls[k] && !((a.src[(long)k * words + w] >> lane) & 1ull)) v = a.bg;   // (bg is no class: nothing matches after it)
        }
        a.out[px] = v;
    }
}

struct Plan { int band, tw, hx, sw, ntx; };

// The tiling of an H x W image for launches of S sub-iterations; forced > 0: that band height.
//   tile width   the whole row up to kMaxTileWords words
//   band height  2 S rows, at least 16 and at most 64, not more than fits or than the image has, evened out over the bands.  Short
//                bands although the halo then recomputes as many rows as the band owns: more, smaller workgroups fill the chip
//                better than fewer large ones (measured at 16 x 256 x 256 and 2 x 1024 x 1024, DESIGN.md section 3.27: at S = 8,
//                16 rows beat or equal 8, 32 and 64 in seven of eight cases)
// Two copies of the staged tile live in LDS: 2 * (band + 2 S) * sw words; at S = 64 and ten words a row 281 rows fit.
int make_plan(int H, int W, int S, int forced, Plan& p) {
    const int nw = (W + 63) / 64;
    p.tw = nw < kMaxTileWords ? nw : kMaxTileWords;
    p.ntx = (nw + p.tw - 1) / p.tw;
    p.hx = p.ntx > 1 ? 1 : 0;
    p.sw = p.tw + 2 * p.hx;
    const int fit = kLdsWords / (2 * p.sw) - 2 * S;
    if (fit < 1 || forced > fit) return UAPS_ERANGE;
    int band = forced;
    if (forced <= 0) {
        band = 2 * S < 16 ? 16 : (2 * S > 64 ? 64 : 2 * S);
        if (band > fit) band = fit;
        if (band > H) band = H;
        const int nb = (H + band - 1) / band;
        band = (H + nb - 1) / nb;
    }
    p.band = band;
    return UAPS_OK;
}

size_t plane_bytes(int B, int H, int W, int n) { return (size_t)n * B * H * ((W + 63) / 64) * 8; }
}  // namespace

extern "C" int uaps_skeleton_workspace_bytes(int B, int H, int W, int n_classes, size_t* bytes) {
    if (!bytes || B <= 0 || H <= 0 || W <= 0 || n_classes < 1 || n_classes > kMaxSel) return UAPS_EINVAL;
    if (H > kMaxExtent || W > kMaxExtent || (double)B * H * W * 8.0 >= kTooBig) return UAPS_ERANGE;
    const double need = 2.0 * n_classes * (double)B * H * ((W + 63) / 64) * 8.0 + 4.0 * B + 1024.0;
    if (need >= kTooBig) return UAPS_ERANGE;
    *bytes = 2 * align256(plane_bytes(B, H, W, n_classes)) + align256((size_t)B * 4);
    return UAPS_OK;
}

extern "C" int uaps_skeleton_band_rows(int H, int W, int n_planes, int S, int* rows) {
    if (!rows || H <= 0 || W <= 0 || n_planes < 2 || n_planes > kMaxSel + 1) return UAPS_EINVAL;
    if (S != 0 && (S < 2 || S > kMaxS || (S & 1))) return UAPS_EINVAL;
    if (H > kMaxExtent || W > kMaxExtent) return UAPS_ERANGE;
    Plan p;
    const int rc = make_plan(H, W, S ? S : kDefaultS, 0, p);
    if (rc) return rc;
    *rows = p.band;
    return UAPS_OK;
}

extern "C" int uaps_skeletonize(const uaps_skeleton_call* call) {
    uaps_skeleton_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.mask || !c.out || !c.converged || !c.workspace || (const void*)c.out == (const void*)c.mask) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0) return UAPS_EINVAL;
    if (c.n_classes < 1 || c.n_classes > kMaxSel || c.band_rows < 0) return UAPS_EINVAL;
    if (c.max_iters < 1 || c.max_iters > UAPS_SKEL_MAX_ITERS) return UAPS_EINVAL;
    if (c.sub_iters != 0 && (c.sub_iters < 2 || c.sub_iters > kMaxS || (c.sub_iters & 1))) return UAPS_EINVAL;
    if (!uaps::distinct_classes(c.classes, c.n_classes, c.background)) return UAPS_EINVAL;
    size_t need = 0;
    int rc = uaps_skeleton_workspace_bytes(c.B, c.H, c.W, c.n_classes, &need);
    if (rc) return rc;
    const int S = c.sub_iters ? c.sub_iters : kDefaultS;
    Plan p;
    rc = make_plan(c.H, c.W, S, c.band_rows, p);
    if (rc) return rc;
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, need)) return UAPS_EWORKSPACE;

    SkelArgs a;
    memset(&a, 0, sizeof a);
    a.B = c.B; a.H = c.H; a.W = c.W; a.nw = (c.W + 63) / 64;
    a.n = c.n_classes; a.S = S;
    a.band = p.band; a.R = p.band + 2 * S;
    a.tw = p.tw; a.sw = p.sw; a.hx = p.hx; a.ntx = p.ntx; a.nby = (c.H + p.band - 1) / p.band;
    for (int k = 0; k < c.n_classes; ++k) a.cls[k] = c.classes[k];
    a.bg = c.background;
    a.mask = (const long long*)c.mask; a.out = (long long*)c.out;
    const size_t half = align256(plane_bytes(c.B, c.H, c.W, c.n_classes));
    char* ws = (char*)c.workspace;
    u64* buf[2] = {reinterpret_cast<u64*>(ws), reinterpret_cast<u64*>(ws + half)};
    a.last = reinterpret_cast<unsigned*>(ws + 2 * half);
    a.converged = c.converged;

    hipStream_t st = (hipStream_t)c.stream;
    const dim3 block(kThreads);
    const long words = (long)c.B * c.H * a.nw;                                      // of one plane; one wave each below
    const dim3 wgrid(grid_for(words * 64, kMaxGrid));
    const int total = 2 * c.max_iters, launches = (total + S - 1) / S;
    uaps::account_bytes(16.0 * c.B * c.H * c.W + 16.0 * (launches + 1) * (double)c.n_classes * (double)words);
    a.dst = buf[0];
    hipLaunchKernelGGL(skel_pack_kernel, wgrid, block, 0, st, a);
    const size_t lds_bytes = (size_t)2 * a.R * a.sw * 8;                            // <= 64 KiB by make_plan
    const long blocks = (long)c.n_classes * c.B * a.nby * a.ntx;                    // <= 8 * B * H * nw < 2^31
    for (int L = 0; L < launches; ++L) {
        a.launch = L;
        a.s_now = total - L * S < S ? total - L * S : S;
        a.src = buf[L & 1]; a.dst = buf[(L + 1) & 1];
        if (L == 0) UAPS_LAUNCH_MAIN(skel_thin_kernel, dim3((unsigned)blocks), block, lds_bytes, st, a);
        else hipLaunchKernelGGL(skel_thin_kernel, dim3((unsigned)blocks), block, lds_bytes, st, a);
    }
    a.src = buf[launches & 1]; a.dst = nullptr;
    hipLaunchKernelGGL(skel_check_kernel, dim3(grid_for((long)c.n_classes * words, kMaxGrid)), block, 0, st, a);
    hipLaunchKernelGGL(skel_unpack_kernel, wgrid, block, 0, st, a);
    return (int)hipGetLastError();
}

// ---- uaps_skeleton_stats ----------------------------------------------------------------------------------------------------------
namespace {
constexpr int kCols = UAPS_SKEL_COLUMNS, kMaxCol = 5;   // d2max: the table's one maximum column (table_flush.hpp)
constexpr int kSpan = 4, kItems = 2, kChunk = kSpan * 64;       // groups of 64 pixels an item, items a wave
constexpr int kLdsRows = uaps::table::kLdsRows;
constexpr int kField = 12;                              // bits of a count in the packed word
constexpr u64 kFieldMask = (1ull << kField) - 1;

struct StatArgs {
    int H, W, M, nchunks, bpi, n;                       // bpi: workgroups an image
    long items;                                         // H * nchunks, of one image
    long long cls[kMaxSel];
    const int* labels;
    const long long* skel;
    const int* plane;
    u64* table;
};

__global__ __launch_bounds__(kThreads) void skeleton_zero_kernel(u64* table, long n) { uaps::table::table_zero(table, n); }

struct StatAcc { u64 q, ps; unsigned pm; };

template <bool PLANE>
__device__ __forceinline__ void stat_send(u64* rows, int k, const StatAcc& r) {
    u64* row = rows + (long)(k - 1) * kCols;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const u64 v = (r.q >> (kField * c)) & kFieldMask;
        if (v) atomicAdd(row + c, v);
    }
    if (PLANE) {
        if (r.pm) atomicMax(row + kMaxCol, (u64)r.pm);
        if (r.ps) atomicAdd(row + kMaxCol + 1, r.ps);
    }
}

template <bool PLANE, bool LDS>
__global__ __launch_bounds__(kThreads) void skeleton_stats_kernel(StatArgs a) {
    extern __shared__ u64 acc[];                        // LDS form: [M][7]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / a.bpi, blk = blockIdx.x - b * a.bpi;
    const int words = a.M * kCols;
    u64* const out = a.table + (long)b * words;
    u64* const rows = LDS ? acc : out;
    if (LDS) table_lds_zero(acc, words);
    const long HW = (long)a.H * a.W;
    const int* lab = a.labels + (long)b * HW;
    const long long* sk = a.skel + (long)b * HW;
    const int* pl = PLANE ? a.plane + (long)b * HW : nullptr;
    const unsigned M = (unsigned)a.M;
    long long cls[kMaxSel];
#pragma unroll
    for (int k = 0; k < kMaxSel; ++k) cls[k] = a.cls[k];
    const int n = a.n;
    // the defect whose skeleton pixel (y, x) is, 0 where it is none; (y, x) inside the image
    auto defect = [&](int y, int x) {
        const long p = (long)y * a.W + x;
        const int v = lab[p];
        if ((unsigned)v - 1u >= M) return 0;            // negative and huge labels alike: no row
        const long long s = sk[p];
        bool sel = false;
#pragma unroll
        for (int k = 0; k < kMaxSel; ++k) sel |= k < n && s == cls[k];
        return sel ? v : 0;
    };

    for (int it = 0; it < kItems; ++it) {
        const long item = ((long)blk * kWaves + wave) * kItems + it;
        if (item >= a.items) break;                     // (wave-uniform; the barrier of the flush is outside the loop)
        const int y = (int)(item / a.nchunks), ch = (int)(item - (long)y * a.nchunks);
        const bool has_up = y > 0, has_dn = y < a.H - 1;
        for (int g = 0; g < kSpan; ++g) {
            const int xg = ch * kChunk + g * 64;
            if (xg >= a.W) break;                       // (wave-uniform)
            const int x = xg + lane;
            const bool valid = x < a.W;
            int up = 0, mid = 0, dn = 0, ev = 0;
            if (valid) {
                mid = defect(y, x);
                if (has_up) up = defect(y - 1, x);
                if (has_dn) dn = defect(y + 1, x);
            }
            if (lane < 6) {                             // lanes 0..2: column xg - 1 of rows y - 1, y, y + 1; lanes 3..5: column xg + 64
                const int r = lane < 3 ? lane : lane - 3, ry = y - 1 + r, cx = lane < 3 ? xg - 1 : xg + 64;
                if (ry >= 0 && ry < a.H && cx >= 0 && cx < a.W) ev = defect(ry, cx);
            }
            const int e0 = __shfl(ev, 0, 64), e1 = __shfl(ev, 1, 64), e2 = __shfl(ev, 2, 64);
            const int e3 = __shfl(ev, 3, 64), e4 = __shfl(ev, 4, 64), e5 = __shfl(ev, 5, 64);
            const int up_l = __shfl_up(up, 1, 64), mid_l = __shfl_up(mid, 1, 64), dn_l = __shfl_up(dn, 1, 64);
            const int up_r = __shfl_down(up, 1, 64), mid_r = __shfl_down(mid, 1, 64), dn_r = __shfl_down(dn, 1, 64);
            const int k = mid;
            // "is linked", clockwise from the north
            const bool N = up == k, NE = (lane == 63 ? e3 : up_r) == k, E = (lane == 63 ? e4 : mid_r) == k;
            const bool SE = (lane == 63 ? e5 : dn_r) == k, S = dn == k, SW = (lane == 0 ? e2 : dn_l) == k;
            const bool Wl = (lane == 0 ? e1 : mid_l) == k, NW = (lane == 0 ? e0 : up_l) == k;
            u64 q = 0ull, ps = 0ull;
            unsigned pm = 0u;
            if (k > 0) {
                const int links = N + NE + E + SE + S + SW + Wl + NW;
                const int rises = (!N && NE) + (!NE && E) + (!E && SE) + (!SE && S) + (!S && SW) + (!SW && Wl) + (!Wl && NW) + (!NW && N);
                const int orth = E + S;                                             // the links this pixel is the raster-first end of
                const int diag = (SE && !E && !S) + (SW && !Wl && !S);
                q = 1ull | ((u64)orth << kField) | ((u64)diag << (2 * kField)) | ((u64)(links == 1) << (3 * kField)) |
                    ((u64)(rises >= 3) << (4 * kField));
                if (PLANE) {
                    const int p = pl[(long)y * a.W + x];
                    pm = p > 0 ? (unsigned)p : 0u;
                    ps = pm;
                }
            }
            const int prev = __shfl_up(k, 1, 64);
            const bool head = lane == 0 || prev != k;
            const unsigned long long heads = __ballot(head);
            const int end = run_end(heads, lane);
            // over [lane, end]: after the step of width o a lane holds what min(2 o, end - lane + 1) lanes hold
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 tq = __shfl_down(q, o, 64);
                const u64 ts = PLANE ? __shfl_down(ps, o, 64) : 0ull;
                const unsigned tm = PLANE ? __shfl_down(pm, o, 64) : 0u;
                if (lane + o <= end) { q += tq; ps += ts; pm = tm > pm ? tm : pm; }
            }
            const StatAcc mine = {q, ps, pm};
            if (head && k > 0) stat_send<PLANE>(rows, k, mine);
        }
    }
    if (LDS) table_lds_flush<kCols, kMaxCol>(acc, out, words);
}
}  // namespace

extern "C" int uaps_skeleton_stats(const uaps_skeleton_stats_call* call) {
    uaps_skeleton_stats_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.labels || !c.skel || !c.table) return UAPS_EINVAL;
    if ((const void*)c.table == (const void*)c.labels || (const void*)c.table == (const void*)c.skel) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0 || c.max_instances < 1 || c.n_classes < 1 || c.n_classes > kMaxSel) return UAPS_EINVAL;
    if (c.H > UAPS_SHAPE_MAX_EXTENT || c.W > UAPS_SHAPE_MAX_EXTENT) return UAPS_ERANGE;
    if ((double)c.H * c.W >= kTooBig || (double)c.B * c.H * c.W * 8.0 >= kTooBig) return UAPS_ERANGE;
    if ((double)c.B * c.max_instances * (8.0 * kCols) >= kTooBig) return UAPS_ERANGE;

    hipStream_t st = (hipStream_t)c.stream;
    const long words = (long)c.B * c.max_instances * kCols;
    uaps::account_bytes((double)c.B * c.H * c.W * (c.plane ? 16.0 : 12.0) + 8.0 * (double)words);
    StatArgs a;
    memset(&a, 0, sizeof a);
    a.H = c.H; a.W = c.W; a.M = c.max_instances; a.nchunks = (c.W + kChunk - 1) / kChunk; a.n = c.n_classes;
    a.items = (long)c.H * a.nchunks;                            // <= 16384 * 64
    a.bpi = (int)((a.items + kWaves * kItems - 1) / (kWaves * kItems));
    for (int k = 0; k < c.n_classes; ++k) a.cls[k] = c.classes[k];
    a.labels = c.labels; a.skel = (const long long*)c.skel; a.plane = c.plane; a.table = reinterpret_cast<u64*>(c.table);
    const dim3 grid((unsigned)((long)c.B * a.bpi)), block(kThreads);       // <= B * H * nchunks / 8 + B < 2^26
    hipLaunchKernelGGL(skeleton_zero_kernel, dim3(grid_for(words, uaps::table::kMaxGrid)), block, 0, st, a.table, words);
    if (c.max_instances <= kLdsRows) {
        const size_t bytes = (size_t)c.max_instances * kCols * sizeof(u64);
        if (c.plane) UAPS_LAUNCH_MAIN((skeleton_stats_kernel<true, true>), grid, block, bytes, st, a);
        else UAPS_LAUNCH_MAIN((skeleton_stats_kernel<false, true>), grid, block, bytes, st, a);
    } else {
        if (c.plane) UAPS_LAUNCH_MAIN((skeleton_stats_kernel<true, false>), grid, block, 0, st, a);
        else UAPS_LAUNCH_MAIN((skeleton_stats_kernel<false, false>), grid, block, 0, st, a);
    }
    return (int)hipGetLastError();
}
