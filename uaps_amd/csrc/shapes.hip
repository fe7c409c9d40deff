// Defect shape descriptors for gfx950 (include/uaps_hip.h, uaps_shape_descriptors): per component of a label image the raw moments
// up to order two, Gray's bit-quad counts and the maximum and sum of an optional integer plane, as exact 64-bit integers.
//
// Two launches: shape_zero_kernel zeroes the table, shape_accumulate_kernel<PLANE, LDS> makes one pass over the labels.
//   Work     An item is one row y of one image and one chunk of SPAN * 64 columns of it; a wave walks its item in groups of 64
//            pixels, a workgroup holds kWaves * kItems consecutive items of ONE image.  SPAN is 4 in the LDS form (more, shorter items:
//            measured 42 -> 17 us at 2 x 1024^2) and 16 in the direct form (a component that fills rows sends a quarter of the atomics
//            to its one row: measured 99 us against 305 us with 4).
//   Loading  A lane loads rows y - 1, y, y + 1 at its column (three coalesced loads); lanes 0..5 also load the three words left of
//            the group and the three right of it, and the other neighbours come from shuffles.  What lies outside the image, and
//            every label outside [1, M], reads as 0: such a label has no row and is "not k" for every component.
//   Quads    A pixel labelled k OWNS a 2 x 2 window for k when no earlier pixel of the window, in raster order, is labelled k; the
//            owner classifies the window from its own eight neighbours.  So every (window, component) pair is counted exactly once,
//            by a lane whose own label is k, and the four counts travel with the lane as one packed word (16 bits each: a wave's item
//            adds at most 4 * 16 * 64 = 4096 to a field).
//   Runs     Everything is reduced over runs of equal labels along the row (cc_common.hpp's run_end and a segmented __shfl_down);
//            a group that is one run of one component is carried on by the wave to the next group.  The moments of a run [x0, x0 + n)
//            in row y are closed forms and need no shuffle.
//   Flush    LDS == true: the runs' first lanes add into the workgroup's copy of the image's table in LDS (M * 88 bytes), and the
//            workgroup then sends the non-zero words to the table with 64-bit atomics.  LDS == false (M above kLdsRows): the
//            first lanes send them directly.  atomicAdd, and atomicMax for pmax, on non-negative integers: two runs and both
//            forms give the same bits.
// No workspace, no float, no host synchronisation, no scratch.
#include "cc_common.hpp"
#include "table_flush.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::u64;
using uaps::cc::run_end;
using uaps::table::table_lds_zero;
using uaps::table::table_lds_flush;

constexpr int kCols = UAPS_SHAPE_COLUMNS;
constexpr int kSpanLds = 4, kSpanDirect = uaps::cc::kSpan;      // groups of 64 pixels an item, per flush form
constexpr int kItems = 2;                               // items a wave
constexpr int kLdsRows = uaps::table::kLdsRows;
constexpr int kMaxGrid = uaps::table::kMaxGrid;
constexpr int kMaxCol = 9;                              // pmax: the table's one maximum column (table_flush.hpp)

struct ShapeArgs {
    int H, W, M, nchunks, bpi;                          // bpi: workgroups an image
    long items;                                         // H * nchunks, of one image
    const int* labels;
    const int* plane;
    u64* table;
};

// the sum of the squares of 0 .. m (m >= -1)
__device__ __forceinline__ long long squares_to(long long m) { return m * (m + 1) * (2 * m + 1) / 6; }

__global__ __launch_bounds__(kThreads) void shape_zero_kernel(u64* table, long n) { uaps::table::table_zero(table, n); }

struct RunAcc { int x0, n; u64 q, ps; unsigned pm; };

// one run [x0, x0 + n) of component k in row y -> the 11 words of row k - 1 of `rows` (LDS or global); zero words are not sent
template <bool PLANE>
__device__ __forceinline__ void shape_send(u64* rows, int k, int y, const RunAcc& r) {
    u64* row = rows + (long)(k - 1) * kCols;
    const long long n = r.n, x0 = r.x0, yy = y;
    const long long sx = n * (2 * x0 + n - 1) / 2;
    const long long sxx = squares_to(x0 + n - 1) - squares_to(x0 - 1);
    const u64 v[9] = {(u64)(yy * n), (u64)sx, (u64)(yy * yy * n), (u64)(yy * sx), (u64)sxx,
                      r.q & 0xffffull, (r.q >> 16) & 0xffffull, (r.q >> 32) & 0xffffull, r.q >> 48};
#pragma unroll
    for (int c = 0; c < 9; ++c)
        if (v[c]) atomicAdd(row + c, v[c]);
    if (PLANE) {
        if (r.pm) atomicMax(row + kMaxCol, (u64)r.pm);
        if (r.ps) atomicAdd(row + 10, r.ps);
    }
}

template <bool PLANE, bool LDS>
__global__ __launch_bounds__(kThreads) void shape_accumulate_kernel(ShapeArgs a) {
    extern __shared__ u64 acc[];                        // LDS form: [M][11]
    constexpr int kSpan = LDS ? kSpanLds : kSpanDirect, kChunk = kSpan * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / a.bpi, blk = blockIdx.x - b * a.bpi;
    const int words = a.M * kCols;
    u64* const out = a.table + (long)b * words;
    u64* const rows = LDS ? acc : out;
    if (LDS) table_lds_zero(acc, words);
    const long HW = (long)a.H * a.W;
    const int* lab = a.labels + (long)b * HW;
    const int* pl = PLANE ? a.plane + (long)b * HW : nullptr;
    const unsigned M = (unsigned)a.M;
    auto norm = [M](int v) { return (unsigned)v - 1u < M ? v : 0; };           // negative and huge labels alike: no row

    for (int it = 0; it < kItems; ++it) {
        const long item = ((long)blk * kWaves + wave) * kItems + it;
        if (item >= a.items) break;                     // (wave-uniform; the barrier below is outside the loop)
        const int y = (int)(item / a.nchunks), ch = (int)(item - (long)y * a.nchunks);
        const bool has_up = y > 0, has_dn = y < a.H - 1;
        const int* mid_row = lab + (long)y * a.W;
        int pend_k = 0;                                 // whole groups of one component, carried by the wave; lane 0 flushes
        RunAcc pend = {0, 0, 0ull, 0ull, 0u};
        for (int g = 0; g < kSpan; ++g) {
            const int xg = ch * kChunk + g * 64;
            if (xg >= a.W) break;                       // (wave-uniform)
            const int x = xg + lane;
            const bool valid = x < a.W;
            int up = 0, mid = 0, dn = 0, ev = 0;
            if (valid) {
                mid = norm(mid_row[x]);
                if (has_up) up = norm(mid_row[x - a.W]);
                if (has_dn) dn = norm(mid_row[x + a.W]);
            }
            if (lane < 6) {                             // lanes 0..2: column xg - 1 of rows y - 1, y, y + 1; lanes 3..5: column xg + 64
                const int r = lane < 3 ? lane : lane - 3, ry = y - 1 + r, cx = lane < 3 ? xg - 1 : xg + 64;
                if (ry >= 0 && ry < a.H && cx >= 0 && cx < a.W) ev = norm(lab[(long)ry * a.W + cx]);
            }
            const int e0 = __shfl(ev, 0, 64), e1 = __shfl(ev, 1, 64), e2 = __shfl(ev, 2, 64);
            const int e3 = __shfl(ev, 3, 64), e4 = __shfl(ev, 4, 64), e5 = __shfl(ev, 5, 64);
            const int up_l = __shfl_up(up, 1, 64), mid_l = __shfl_up(mid, 1, 64), dn_l = __shfl_up(dn, 1, 64);
            const int up_r = __shfl_down(up, 1, 64), mid_r = __shfl_down(mid, 1, 64), dn_r = __shfl_down(dn, 1, 64);
            const int k = mid;
            // the eight neighbours, "carries my label":  A B C / D . E / F G H
            const bool A = (lane == 0 ? e0 : up_l) == k, B = up == k, Cc = (lane == 63 ? e3 : up_r) == k;
            const bool D = (lane == 0 ? e1 : mid_l) == k, E = (lane == 63 ? e4 : mid_r) == k;
            const bool F = (lane == 0 ? e2 : dn_l) == k, G = dn == k, Hh = (lane == 63 ? e5 : dn_r) == k;
            u64 q = 0ull, ps = 0ull;
            unsigned pm = 0u;
            if (k > 0) {
                constexpr u64 Q1 = 1ull, Q2 = 1ull << 16, Q3 = 1ull << 32, QD = 1ull << 48;
                if (!A && !B && !D) q += Q1;                               // the window whose last pixel I am: I own it alone
                if (!B && !Cc) q += E ? Q2 : Q1;                           // B C / . E
                if (!D) q += F ? (G ? Q3 : QD) : (G ? Q2 : Q1);            // D . / F G
                const int n = (E ? 1 : 0) + (G ? 1 : 0) + (Hh ? 1 : 0);    // . E / G H: I am its first pixel
                if (n == 0) q += Q1;
                else if (n == 1) q += Hh ? QD : Q2;
                else if (n == 2) q += Q3;
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
            const RunAcc mine = {x, end - lane + 1, q, ps, pm};
            const int k0 = __shfl(k, 0, 64);
            if (heads == 1ull && k0 > 0) {              // the group is one run of one component (so all 64 lanes are inside the row)
                if (pend_k == k0) {
                    pend.n += 64; pend.q += mine.q; pend.ps += mine.ps; pend.pm = mine.pm > pend.pm ? mine.pm : pend.pm;
                } else {
                    if (pend_k > 0 && lane == 0) shape_send<PLANE>(rows, pend_k, y, pend);
                    pend_k = k0; pend = mine;
                }
                continue;
            }
            if (pend_k > 0 && lane == 0) shape_send<PLANE>(rows, pend_k, y, pend);
            pend_k = 0;
            if (head && k > 0) shape_send<PLANE>(rows, k, y, mine);
        }
        if (pend_k > 0 && lane == 0) shape_send<PLANE>(rows, pend_k, y, pend);
    }
    if (LDS) table_lds_flush<kCols, kMaxCol>(acc, out, words);
}
}  // namespace

extern "C" int uaps_shape_descriptors(const uaps_shape_call* call) {
    uaps_shape_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.labels || !c.table || (const void*)c.table == (const void*)c.labels) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0 || c.max_instances < 1) return UAPS_EINVAL;
    if (c.H > UAPS_SHAPE_MAX_EXTENT || c.W > UAPS_SHAPE_MAX_EXTENT) return UAPS_ERANGE;
    if ((double)c.H * c.W >= kTooBig || (double)c.B * c.H * c.W * 8.0 >= kTooBig) return UAPS_ERANGE;
    if ((double)c.B * c.max_instances * (8.0 * kCols) >= kTooBig) return UAPS_ERANGE;

    hipStream_t st = (hipStream_t)c.stream;
    const long words = (long)c.B * c.max_instances * kCols;
    uaps::account_bytes((double)c.B * c.H * c.W * (c.plane ? 8.0 : 4.0) + 8.0 * (double)words);
    ShapeArgs a;
    memset(&a, 0, sizeof a);
    const bool lds = c.max_instances <= kLdsRows;
    const int chunk = 64 * (lds ? kSpanLds : kSpanDirect);
    a.H = c.H; a.W = c.W; a.M = c.max_instances; a.nchunks = (c.W + chunk - 1) / chunk;
    a.items = (long)c.H * a.nchunks;                            // <= 16384 * 64
    a.bpi = (int)((a.items + kWaves * kItems - 1) / (kWaves * kItems));
    a.labels = c.labels; a.plane = c.plane; a.table = reinterpret_cast<u64*>(c.table);
    const dim3 grid((unsigned)((long)c.B * a.bpi)), block(kThreads);       // <= B * H * nchunks / 8 + B < 2^26
    hipLaunchKernelGGL(shape_zero_kernel, dim3(grid_for(words, kMaxGrid)), block, 0, st, a.table, words);
    if (lds) {
        const size_t bytes = (size_t)c.max_instances * kCols * sizeof(u64);
        if (c.plane) UAPS_LAUNCH_MAIN((shape_accumulate_kernel<true, true>), grid, block, bytes, st, a);
        else UAPS_LAUNCH_MAIN((shape_accumulate_kernel<false, true>), grid, block, bytes, st, a);
    } else {
        if (c.plane) UAPS_LAUNCH_MAIN((shape_accumulate_kernel<true, false>), grid, block, 0, st, a);
        else UAPS_LAUNCH_MAIN((shape_accumulate_kernel<false, false>), grid, block, 0, st, a);
    }
    return (int)hipGetLastError();
}
