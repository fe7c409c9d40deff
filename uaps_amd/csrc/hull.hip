// Defect convex hulls for gfx950 (include/uaps_hip.h, uaps_hull_descriptors): per component of a label image the convex hull of its
// pixel squares and, from the hull's strict vertices, the shoelace area, the farthest pair, the minimum caliper width and the
// minimum-area rectangle, as exact 64-bit integers.  A pixel (y, x) is the closed square [x, x + 1] x [y, y + 1], so the vertices lie
// on the corner lattice 0..W x 0..H; the hull order starts at the smallest vertex (y, then x) and runs along the top edge towards
// +x, and with the edge vector e = (ex, ey) from v_i to v_{i+1} every hull point p has c(p) = ex (py - vy) - ey (px - vx) >= 0.
//
// Three launches over a workspace of B * M * (H + 1) pairs of 32-bit words:
//   hull_zero_kernel      zeroes the workspace.
//   hull_extents_kernel   one pass over the labels, laid out like shape_accumulate_kernel: an item is one row y and one chunk of
//                         kSpan * 64 columns, a wave walks it in groups of 64 pixels, runs of equal labels come from run_end, a group
//                         that is one run of one component is carried on by the wave.  A run [x0, x0 + n) of component k in row y
//                         raises the row's pair (W - x0, x0 + n) and the component's pair (H - y, y + 1).  BOTH words are maxima
//                         over zeroed memory (the minimum is stored inverted), so zero means "no pixel", one zeroing pass serves
//                         both, and integer atomicMax alone gives the same bits from run to run.  A word is read first and the
//                         atomic is skipped where it would change nothing: a component that fills rows would otherwise send every
//                         run of the image to its ONE pair of row-range words.
//   hull_measure_kernel   one workgroup per (image, component).  Two uniform loads say whether it has a pixel; if not, the row is
//                         written as zeros and the workgroup is done.  Otherwise the lattice lines Y = ymin .. ymax + 1 get their
//                         points L[Y] = min(xmin[Y-1], xmin[Y]) and R[Y] = max(xmax[Y-1], xmax[Y]) + 1 as packed words
//                         (Y << 16 | X, which order as (y, x) does) in LDS, 8 bytes a line; a line neither of whose rows carries
//                         the label (a label need not be connected) is marked absent.  All lanes first drop every point that does
//                         not turn strictly between its two neighbours (the lines along a straight side).  Wave 0 then reduces the
//                         right chain downwards and wave 1 the left chain upwards with the monotone-chain rule, in place: a wave
//                         reads 64 points at a time, a ballot names the present ones, and the stack work on those is wave-uniform
//                         (the stack never passes the read position; its top two points stay in registers); a point is kept only
//                         where the turn is strict.  The cyclic vertex list is the right stack followed by the left one.  Then all lanes
//                         share the shoelace sum, the pairs (for the farthest pair) and the edges (for each edge a loop over all
//                         vertices gives the largest c and the range of d(p) = ex (px - vx) + ey (py - vy)); the two
//                         minimisations compare fractions by cross-multiplication in 128-bit integers, ties to the lowest edge.
// No float, no host synchronisation, no scratch; LDS 8 (H + 1) bytes + 128.
#include "cc_common.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256; using uaps::u64;
using uaps::cc::run_end;

constexpr int kCols = UAPS_HULL_COLUMNS;
constexpr int kMaxExtent = UAPS_HULL_MAX_EXTENT;
constexpr int kSpan = uaps::cc::kSpan, kChunk = kSpan * 64;     // groups of 64 pixels an item
constexpr int kItems = 2;                                       // items a wave
constexpr int kMaxGrid = 1 << 16;
constexpr unsigned kAbsent = 0xffffffffu;
constexpr int kNoEdge = 0x7fffffff;
typedef unsigned __int128 u128;

struct HullArgs {
    int H, W, M, nchunks, bpi;                          // bpi: workgroups an image (extents pass)
    long items;                                         // H * nchunks, of one image
    const int* labels;
    unsigned* ext;                                      // [B][M][H + 1][2]: rows 0..H-1 (W - xmin, xmax + 1); row H (H - ymin, ymax + 1)
    long long* table;
};

__global__ __launch_bounds__(kThreads) void hull_zero_kernel(u64* ws, long n) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) ws[i] = 0ull;
}

// *p = max(*p, v).  The words only ever grow inside a launch, so a stale read costs an atomic, never a wrong value.
__device__ __forceinline__ void raise(unsigned* p, unsigned v) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(p, v);
}

// one run [x0, x0 + n) of component k in row y; img: the image's part of the workspace
__device__ __forceinline__ void extent_send(const HullArgs& a, unsigned* img, int k, int y, int x0, int n) {
    unsigned* d = img + (long)(k - 1) * (a.H + 1) * 2;
    raise(d + 2 * y, (unsigned)(a.W - x0));
    raise(d + 2 * y + 1, (unsigned)(x0 + n));
    raise(d + 2 * a.H, (unsigned)(a.H - y));
    raise(d + 2 * a.H + 1, (unsigned)(y + 1));
}

__global__ __launch_bounds__(kThreads) void hull_extents_kernel(HullArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / a.bpi, blk = blockIdx.x - b * a.bpi;
    const int* lab = a.labels + (long)b * a.H * a.W;
    unsigned* img = a.ext + (long)b * a.M * (a.H + 1) * 2;
    const unsigned M = (unsigned)a.M;
    for (int it = 0; it < kItems; ++it) {
        const long item = ((long)blk * kWaves + wave) * kItems + it;
        if (item >= a.items) break;                     // (wave-uniform)
        const int y = (int)(item / a.nchunks), ch = (int)(item - (long)y * a.nchunks);
        const int* row = lab + (long)y * a.W;
        int pend_k = 0, pend_x0 = 0, pend_n = 0;        // whole groups of one component, carried by the wave; lane 0 sends
        for (int g = 0; g < kSpan; ++g) {
            const int xg = ch * kChunk + g * 64;
            if (xg >= a.W) break;                       // (wave-uniform)
            const int x = xg + lane;
            int k = 0;
            if (x < a.W) {
                const int v = row[x];
                k = (unsigned)v - 1u < M ? v : 0;       // negative and huge labels alike: no row
            }
            const int prev = __shfl_up(k, 1, 64);
            const bool head = lane == 0 || prev != k;
            const unsigned long long heads = __ballot(head);
            const int end = run_end(heads, lane);
            const int k0 = __shfl(k, 0, 64);
            if (heads == 1ull && k0 > 0) {              // the group is one run of one component (so all 64 lanes are inside the row)
                if (pend_k == k0) {
                    pend_n += 64;
                } else {
                    if (pend_k > 0 && lane == 0) extent_send(a, img, pend_k, y, pend_x0, pend_n);
                    pend_k = k0; pend_x0 = xg; pend_n = 64;
                }
                continue;
            }
            if (pend_k > 0 && lane == 0) extent_send(a, img, pend_k, y, pend_x0, pend_n);
            pend_k = 0;
            if (head && k > 0) extent_send(a, img, k, y, x, end - lane + 1);
        }
        if (pend_k > 0 && lane == 0) extent_send(a, img, pend_k, y, pend_x0, pend_n);
    }
}

// a -> b -> c, three points in hull order: does b turn strictly, c_ab(c) > 0?  (|.| <= 2 * 4096^2)
__device__ __forceinline__ bool strict_turn(unsigned a, unsigned b, unsigned c) {
    const int ax = (int)(a & 0xffffu), ay = (int)(a >> 16), bx = (int)(b & 0xffffu), by = (int)(b >> 16);
    const int cx = (int)(c & 0xffffu), cy = (int)(c >> 16);
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) > 0;
}

// The monotone-chain rule over the n points P[start], P[start + dir], ... (absent points skipped), in place, by ONE WAVE: the stack's
// slot s is P[start + dir * s], never beyond the points already read.  The wave reads 64 points at a time and a ballot names the
// present ones; each of those is then handled by all lanes alike (every value below is wave-uniform, and every lane stores the same
// word to the same slot, so a lane reads back what it wrote itself).  b is kept between a and c only where the turn a -> b -> c is
// strict.  Returns the number of points kept.
__device__ __forceinline__ int chain_reduce(unsigned* P, int n, int start, int dir, int lane) {
    int s = 0;
    unsigned a = 0u, b = 0u;                            // slots s - 2 and s - 1
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const unsigned mine = j < n ? P[start + dir * j] : kAbsent;
        unsigned long long todo = __ballot(mine != kAbsent);
        while (todo) {
            const unsigned c = __shfl(mine, __builtin_ctzll(todo), 64);
            todo &= todo - 1ull;
            while (s >= 2 && !strict_turn(a, b, c)) {
                --s;
                b = a;
                if (s >= 2) a = P[start + dir * (s - 2)];
            }
            P[start + dir * s] = c;                     // (s <= the number of points read before c)
            a = b; b = c; ++s;
        }
    }
    return s;
}

__device__ __forceinline__ u64 block_max(u64 v, u64* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const u64 t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    __syncthreads();                                    // (red may still be read from the reduction before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = red[w] > r ? red[w] : r;
    return r;
}

__device__ __forceinline__ long long block_sum(long long v, u64* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (u64)v;
    __syncthreads();
    long long r = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) r += (long long)red[w];
    return r;
}

// an edge's value num / den with its hull index; (1, 0, kNoEdge) is "no edge" and loses against every edge
struct Frac { u64 num; unsigned den; int idx; };
__device__ __forceinline__ bool frac_before(const Frac& p, const Frac& q) {         // p wins against q
    const u128 l = (u128)p.num * q.den, r = (u128)q.num * p.den;
    return l < r || (l == r && p.idx < q.idx);
}

// the index of the winning edge, in every thread
__device__ __forceinline__ int block_best_edge(Frac f, u64* rn, unsigned* rd, int* ri) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        Frac t;
        t.num = __shfl_xor(f.num, o, 64); t.den = __shfl_xor(f.den, o, 64); t.idx = __shfl_xor(f.idx, o, 64);
        if (frac_before(t, f)) f = t;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { rn[threadIdx.x >> 6] = f.num; rd[threadIdx.x >> 6] = f.den; ri[threadIdx.x >> 6] = f.idx; }
    __syncthreads();
    Frac r = {rn[0], rd[0], ri[0]};
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        const Frac t = {rn[w], rd[w], ri[w]};
        if (frac_before(t, r)) r = t;
    }
    return r.idx;
}

__global__ __launch_bounds__(kThreads) void hull_measure_kernel(HullArgs a) {
    extern __shared__ unsigned chain[];                 // [2][n]: the right chain's points, then the left chain's
    __shared__ u64 red[kWaves];
    __shared__ unsigned red_den[kWaves];
    __shared__ int red_idx[kWaves];
    __shared__ int kept[2];
    const int t = threadIdx.x;
    const long dk = blockIdx.x;                         // image * M + component - 1
    const unsigned* d = a.ext + dk * (a.H + 1) * 2;
    long long* out = a.table + dk * kCols;
    const unsigned ylo = d[2 * a.H], yhi = d[2 * a.H + 1];
    if (yhi == 0u) {                                    // no pixel carries this label
        if (t < kCols) out[t] = 0;
        return;
    }
    const int y0 = a.H - (int)ylo, y1 = (int)yhi - 1;   // the first and the last row with a pixel
    const int n = y1 - y0 + 2;                          // lattice lines y0 .. y1 + 1;  n <= H + 1
    unsigned* PR = chain;
    unsigned* PL = chain + n;
    for (int i = t; i < n; i += kThreads) {
        const int Y = y0 + i;
        unsigned lo = 0u, hi = 0u;                      // max (W - xmin), max (xmax + 1) over the rows Y - 1 and Y
        if (Y > y0) { lo = d[2 * (Y - 1)]; hi = d[2 * (Y - 1) + 1]; }
        if (Y <= y1) {
            const unsigned l2 = d[2 * Y], h2 = d[2 * Y + 1];
            lo = l2 > lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
        }
        PR[i] = hi ? ((unsigned)Y << 16 | hi) : kAbsent;
        PL[i] = hi ? ((unsigned)Y << 16 | (unsigned)(a.W - (int)lo)) : kAbsent;
    }
    __syncthreads();
    // A point that does not turn strictly between its two lattice-line neighbours is no strict vertex of the hull, whatever becomes
    // of the neighbours: it goes before the serial pass, which then meets the ends of a straight side and not every line along it.
    // (Bit r of a mask: this thread's point t + r * kThreads; n <= 4097 makes at most 17 of them.)
    unsigned drop_r = 0u, drop_l = 0u;
    for (int i = t, r = 0; i < n; i += kThreads, ++r) {
        if (i == 0 || i == n - 1) continue;
        const unsigned ra = PR[i - 1], rb = PR[i], rc = PR[i + 1], la = PL[i + 1], lb = PL[i], lc = PL[i - 1];
        if (ra != kAbsent && rb != kAbsent && rc != kAbsent && !strict_turn(ra, rb, rc)) drop_r |= 1u << r;
        if (la != kAbsent && lb != kAbsent && lc != kAbsent && !strict_turn(la, lb, lc)) drop_l |= 1u << r;
    }
    __syncthreads();
    for (int i = t, r = 0; i < n; i += kThreads, ++r) {
        if (drop_r >> r & 1u) PR[i] = kAbsent;
        if (drop_l >> r & 1u) PL[i] = kAbsent;
    }
    __syncthreads();
    const int lane = t & 63;
    if (t < 64) {                                               // downwards: slots PR[0 ..]
        const int k0 = chain_reduce(PR, n, 0, 1, lane);
        if (t == 0) kept[0] = k0;
    } else if (t < 128) {                                       // upwards: slots PL[n - 1], PL[n - 2], ..
        const int k1 = chain_reduce(PL, n, n - 1, -1, lane);
        if (t == 64) kept[1] = k1;
    }
    __syncthreads();
    const int nr = kept[0], nv = nr + kept[1];
    // cyclic order: the right stack, then the left one; hull vertex i is cyclic vertex i - 1, and vertex 0 the last (the top left)
    auto cv = [&](int j) -> unsigned { return j < nr ? chain[j] : chain[2 * n - 1 + nr - j]; };
    auto hv = [&](int i) -> unsigned { return cv(i == 0 ? nv - 1 : i - 1); };

    long long sum = 0;
    u64 far_key = 0ull;                                 // d^2 << 32 | ~(the smaller point): the largest wins
    unsigned far_hi = kAbsent;                          // the larger point of that pair: the smallest wins
    for (int j = t; j < nv; j += kThreads) {
        const unsigned p = cv(j), q = cv(j + 1 == nv ? 0 : j + 1);
        const int px = (int)(p & 0xffffu), py = (int)(p >> 16), qx = (int)(q & 0xffffu), qy = (int)(q >> 16);
        sum += (long long)(px * qy - qx * py);
        for (int j2 = j + 1; j2 < nv; ++j2) {
            const unsigned r = cv(j2);
            const int dx = (int)(r & 0xffffu) - px, dy = (int)(r >> 16) - py;
            const unsigned lo = p < r ? p : r, hi = p < r ? r : p;
            const u64 key = (u64)(unsigned)(dx * dx + dy * dy) << 32 | (u64)(0xffffffffu - lo);
            if (key > far_key || (key == far_key && hi < far_hi)) { far_key = key; far_hi = hi; }
        }
    }
    const long long area2 = block_sum(sum, red);
    const u64 best_key = block_max(far_key, red);
    const unsigned f1 = 0xffffffffu - (unsigned)block_max(far_key == best_key ? (u64)(0xffffffffu - far_hi) : 0ull, red);
    const unsigned f0 = 0xffffffffu - (unsigned)(best_key & 0xffffffffull);

    Frac wbest = {1ull, 0u, kNoEdge}, rbest = {1ull, 0u, kNoEdge};
    int w_ey = 0, w_ex = 0, w_c = 0, r_y = 0, r_x = 0, r_ey = 0, r_ex = 0, r_dmin = 0, r_dmax = 0, r_c = 0;
    for (int i = t; i < nv; i += kThreads) {
        const unsigned v = hv(i), w = hv(i + 1 == nv ? 0 : i + 1);
        const int vx = (int)(v & 0xffffu), vy = (int)(v >> 16);
        const int ex = (int)(w & 0xffffu) - vx, ey = (int)(w >> 16) - vy;
        int cm = 0, dmin = 0, dmax = 0;                 // (v itself has c = d = 0)
        for (int j = 0; j < nv; ++j) {
            const unsigned p = cv(j);
            const int px = (int)(p & 0xffffu) - vx, py = (int)(p >> 16) - vy;
            const int c = ex * py - ey * px, dd = ex * px + ey * py;               // (|.| <= 2 * 4096^2)
            cm = c > cm ? c : cm; dmin = dd < dmin ? dd : dmin; dmax = dd > dmax ? dd : dmax;
        }
        const unsigned e2 = (unsigned)(ex * ex + ey * ey);
        const Frac wf = {(u64)cm * (u64)cm, e2, i}, rf = {(u64)(dmax - dmin) * (u64)cm, e2, i};
        if (frac_before(wf, wbest)) { wbest = wf; w_ey = ey; w_ex = ex; w_c = cm; }
        if (frac_before(rf, rbest)) { rbest = rf; r_y = vy; r_x = vx; r_ey = ey; r_ex = ex; r_dmin = dmin; r_dmax = dmax; r_c = cm; }
    }
    const int wi = block_best_edge(wbest, red, red_den, red_idx);
    const int ri = block_best_edge(rbest, red, red_den, red_idx);
    if (t == 0) {
        out[0] = nv; out[1] = area2; out[2] = (long long)(best_key >> 32);
        out[3] = f0 >> 16; out[4] = f0 & 0xffffu; out[5] = f1 >> 16; out[6] = f1 & 0xffffu;
    }
    if (wbest.idx == wi) { out[7] = w_ey; out[8] = w_ex; out[9] = w_c; }            // (an edge belongs to one thread)
    if (rbest.idx == ri) {
        out[10] = r_y; out[11] = r_x; out[12] = r_ey; out[13] = r_ex; out[14] = r_dmin; out[15] = r_dmax; out[16] = r_c;
    }
}
}  // namespace

extern "C" int uaps_hull_workspace_bytes(int B, int H, int W, int max_instances, size_t* bytes) {
    if (!bytes || B <= 0 || H <= 0 || W <= 0 || max_instances < 1) return UAPS_EINVAL;
    if (H > kMaxExtent || W > kMaxExtent || (double)B * H * W * 8.0 >= kTooBig) return UAPS_ERANGE;
    const double need = (double)B * max_instances * (H + 1.0) * 8.0 + 256.0;
    if (need >= kTooBig) return UAPS_ERANGE;
    *bytes = align256((size_t)B * max_instances * (size_t)(H + 1) * 8);
    return UAPS_OK;
}

extern "C" int uaps_hull_descriptors(const uaps_hull_call* call) {
    uaps_hull_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.labels || !c.table || !c.workspace || (const void*)c.table == (const void*)c.labels) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0 || c.max_instances < 1) return UAPS_EINVAL;
    size_t need = 0;
    const int rc = uaps_hull_workspace_bytes(c.B, c.H, c.W, c.max_instances, &need);
    if (rc) return rc;
    if ((double)c.B * c.max_instances * (8.0 * kCols) >= kTooBig) return UAPS_ERANGE;
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, need)) return UAPS_EWORKSPACE;

    hipStream_t st = (hipStream_t)c.stream;
    const long defects = (long)c.B * c.max_instances;           // < 2^28 / 17
    uaps::account_bytes((double)c.B * c.H * c.W * 4.0 + 8.0 * kCols * (double)defects);
    HullArgs a;
    memset(&a, 0, sizeof a);
    a.H = c.H; a.W = c.W; a.M = c.max_instances; a.nchunks = (c.W + kChunk - 1) / kChunk;
    a.items = (long)c.H * a.nchunks;                            // <= 4096 * 4
    a.bpi = (int)((a.items + kWaves * kItems - 1) / (kWaves * kItems));
    a.labels = c.labels; a.ext = reinterpret_cast<unsigned*>(c.workspace); a.table = reinterpret_cast<long long*>(c.table);
    const long words = defects * (c.H + 1);                     // 64-bit words of the workspace: < 2^28
    const dim3 block(kThreads);
    hipLaunchKernelGGL(hull_zero_kernel, dim3(grid_for(words, kMaxGrid)), block, 0, st, reinterpret_cast<u64*>(c.workspace), words);
    hipLaunchKernelGGL(hull_extents_kernel, dim3((unsigned)((long)c.B * a.bpi)), block, 0, st, a);      // <= B * H / 2 + B < 2^27
    UAPS_LAUNCH_MAIN(hull_measure_kernel, dim3((unsigned)defects), block, (size_t)(c.H + 1) * 8, st, a);
    return (int)hipGetLastError();
}
