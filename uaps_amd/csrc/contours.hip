// Defect contours for gfx950 (include/uaps_hip.h, uaps_contours_trace / uaps_contours_write): the boundary of every component of a
// label image as closed rings of corner-lattice points.  A pixel (y, x) is the closed square [x, x + 1] x [y, y + 1]; every unit
// side between a pixel of label k (1 <= k <= M) and anything else is a directed edge with k on its right (E, S, W, N = 0..3), named by
// its start vertex and direction; the next edge of a ring leaves the end vertex, and at a saddle vertex (k on exactly the two
// diagonal pixels of the 2 x 2 window) connectivity 8 turns left and connectivity 4 right.  A ring is one cycle of that successor map.
//
// A VERTEX, not a pixel, is the item of the first pass: the 2 x 2 window round vertex (Y, X) decides its up to four outgoing edges
//   E: SE labelled, NE differs      S: SW labelled, SE differs      W: NW labelled, SW differs      N: NE labelled, NW differs
// so edges come out in key order (image, Y (W + 1) + X, direction) and an exclusive scan of the per-vertex counts IS the compaction:
// edge (vertex, dir) has the compact id vbase[vertex] + (the number of the vertex's edges with a lower direction).
//
//   contour_zero_kernel           clears the totals, the round flags and the summary table.
//   contour_sum / _base / _apply  one three-launch exclusive scan of pairs of 64-bit integers, used three times (stage 0, 1, 2 below):
//                                 block sums, one workgroup over the block sums, and the pass that hands every item its prefix.  No
//                                 workgroup waits for another.
//     stage 0  over the vertices: the edge counts -> vbase, the edges' keys, and the ranking's start value (own id, distance 0).
//   contour_link_kernel           one lane an edge: the window at its end vertex and the turn rule name the successor s; the edge
//                                 stores itself as s's PREDECESSOR (the successor map is a permutation: every slot is written once).
//   contour_jump_kernel           pointer doubling BACKWARDS along the ring, one launch a round, double-buffered:
//                                     val[i] = min(val[i], val[p[i]] + 2^r);  p[i] = p[p[i]]        val = (smallest id seen) << 32 | distance
//                                 After round r an edge knows the smallest id among the 2^(r + 1) edges that end with itself and how
//                                 far back it lies; when that covers the ring the id is the ring's leader (its smallest start vertex,
//                                 the ring's start) and the distance IS the edge's rank from the leader.  One phase does the work of
//                                 the usual two (spread the minimum, then cut and rank by Wyllie).  A round that lowers no id raises
//                                 no flag, and every later launch returns at once; nothing is read on the host.
//   contour_rounds_kernel         one lane: how many rounds ran = which buffer holds the result.
//     stage 1  over the edges in key order: (is a leader, the ring's length) -> the ring's index and its first slot in ring order.
//   contour_scatter_kernel        perm[first slot of the ring + rank] = edge: the edges in (ring, rank) order.
//     stage 2  over that order: (the edge turns, its shoelace term) -> the point slot of every turning edge and running area sums.
//   contour_rings_kernel          one lane a ring start: points, length and area2 by differences of the scans, added to the summary row
//                                 of (image, label) with 64-bit integer atomics, in LDS bins first; the totals go to the caller's
//                                 four words.
//   contour_write_kernel          after the host has read the totals and sized the outputs: points, ring_offsets, rings.
// Integers only, no float, 4.5 KiB of LDS at the most (the summary's bins; the scans use 64 bytes), no scratch.  The same bits from run to run: every value is a pure
// function of the labels but the summary's integer sums, whose order does not matter.
#include "call_common.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256; using uaps::u64;
typedef long long i64;

constexpr int kMaxExtent = UAPS_CONTOUR_MAX_EXTENT;
constexpr int kItems = 16, kChunk = kThreads * kItems;          // items of one workgroup of a scan
constexpr int kMaxGrid = 2048;                                  // of the grid-stride passes over the edges
constexpr int kMaxRounds = 32;
constexpr u64 kLow = 0xffffffffull;

struct Pair { i64 a, b; };
__device__ __forceinline__ Pair operator+(const Pair& p, const Pair& q) { return Pair{p.a + q.a, p.b + q.b}; }

struct ContourArgs {
    int B, H, W, M, conn8, rounds;
    long V1, V, Emax;                   // vertices of an image, of the batch; the most edges the batch can have
    const int* labels;
    i64* tot;                           // [0] edges  [1] rings  [2] points  [3] rounds that ran  [4] the sum of all shoelace terms
    int* changed;                       // [kMaxRounds]: round r lowered an id
    Pair* bsum;                         // the scans' block sums
    int* vbase;                         // [V]
    unsigned* ekey;                     // [Emax]: vertex * 4 + direction
    int* prv0;                          // [Emax]: the predecessor
    int* prv[2];                        // [Emax] each: the 2^r-th predecessor, double-buffered
    u64* val[2];                        // [Emax] each
    u64* rec;                           // [Emax], over prv[0] and prv[1] once the rounds are done: at a leader, ring << 32 | first slot
    int* perm;                          // [Emax]: the edge at a slot of ring order
    int* pslot;                         // [Emax]: the turning edges before a slot
    i64* csum;                          // [Emax]: the shoelace terms before a slot
    i64* summary;                       // [B][M][4]
    i64* totals;                        // the caller's [4]
    i64 n_rings, n_points;              // write: what the caller read from `totals`
    int* points;
    int* ring_offsets;
    i64* rings;
};

struct Win { int a, b, c, d; };         // NW, NE, SW, SE of a vertex; 0: outside the frame or no label of [1, M]

__device__ __forceinline__ int own(int v, unsigned M) { return (unsigned)v - 1u < M ? v : 0; }

__device__ __forceinline__ Win window(const ContourArgs& A, const int* lab, int Y, int X) {
    Win w = {0, 0, 0, 0};
    const unsigned M = (unsigned)A.M;
    const bool up = Y > 0, dn = Y < A.H, lf = X > 0, rt = X < A.W;
    if (up && lf) w.a = own(lab[(long)(Y - 1) * A.W + X - 1], M);
    if (up && rt) w.b = own(lab[(long)(Y - 1) * A.W + X], M);
    if (dn && lf) w.c = own(lab[(long)Y * A.W + X - 1], M);
    if (dn && rt) w.d = own(lab[(long)Y * A.W + X], M);
    return w;
}

__device__ __forceinline__ int edge_mask(const Win& w) {
    return (w.d && w.b != w.d ? 1 : 0) | (w.c && w.d != w.c ? 2 : 0) | (w.a && w.c != w.a ? 4 : 0) | (w.b && w.a != w.b ? 8 : 0);
}

__device__ __forceinline__ int edge_label(const Win& w, int dir) { return dir == 0 ? w.d : dir == 1 ? w.c : dir == 2 ? w.a : w.b; }

struct Place { int b, Y, X, dir; };
__device__ __forceinline__ Place place_of(const ContourArgs& A, unsigned key) {
    Place p;
    p.dir = (int)(key & 3u);
    const long g = (long)(key >> 2);
    p.b = (int)(g / A.V1);
    const int v = (int)(g - (long)p.b * A.V1);
    p.Y = v / (A.W + 1);
    p.X = v - p.Y * (A.W + 1);
    return p;
}

// a gathered index that a sound workspace keeps below n; anything else is folded onto the lane's own item and never leaves the arrays
__device__ __forceinline__ long inside(long j, long n, long self) { return (unsigned long)j < (unsigned long)n ? j : self; }

__device__ __forceinline__ int final_buffer(const ContourArgs& A) { return (int)(A.tot[3] & 1); }

// ---- the scan -----------------------------------------------------------------------------------------------------------------------
// exclusive prefix of v over the block; total: the block's sum, in every thread
__device__ __forceinline__ Pair block_scan(Pair v, Pair* red, Pair& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Pair inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const i64 ta = __shfl_up(inc.a, o, 64), tb = __shfl_up(inc.b, o, 64);
        if (lane >= o) { inc.a += ta; inc.b += tb; }
    }
    __syncthreads();                                    // (red may still be read from the scan before)
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    Pair base = {0, 0};
    total = Pair{0, 0};
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const Pair r = red[w];
        if (w < wave) base = base + r;
        total = total + r;
    }
    return Pair{base.a + inc.a - v.a, base.b + inc.b - v.b};
}

template <int S> __device__ __forceinline__ long scan_items(const ContourArgs& A) { return S == 0 ? A.V : (long)A.tot[0]; }

// stage 0, vertex g: (edges, their mask)
// stage 1, edge i in key order: (leads its ring, the ring's length there)
// stage 2, slot s of ring order: (the edge turns, its shoelace term x y' - x' y)
template <int S> __device__ __forceinline__ Pair scan_value(const ContourArgs& A, long i, long n) {
    if (S == 0) {
        const int b = (int)(i / A.V1), v = (int)(i - (long)b * A.V1);
        const int Y = v / (A.W + 1), X = v - Y * (A.W + 1);
        const int m = edge_mask(window(A, A.labels + (long)b * A.H * A.W, Y, X));
        return Pair{(i64)__popc((unsigned)m), (i64)m};
    } else if (S == 1) {
        const u64* val = A.val[final_buffer(A)];
        if ((long)(val[i] >> 32) != i) return Pair{0, 0};
        const long last = inside(A.prv0[i], n, i);
        return Pair{1, (i64)(val[last] & kLow) + 1};
    } else {
        const long e = inside(A.perm[i], n, i);
        const unsigned key = A.ekey[e];
        const Place p = place_of(A, key);
        const int pdir = (int)(A.ekey[inside(A.prv0[e], n, e)] & 3u);
        const int term = p.dir == 0 ? -p.Y : p.dir == 1 ? p.X : p.dir == 2 ? p.Y : -p.X;
        return Pair{pdir != p.dir ? 1 : 0, (i64)term};
    }
}

template <int S> __device__ __forceinline__ void scan_emit(const ContourArgs& A, long i, const Pair& before, const Pair& v) {
    if (S == 0) {
        A.vbase[i] = (int)before.a;
        long id = before.a;
        for (int dir = 0; dir < 4; ++dir) {
            if (!((int)v.b >> dir & 1)) continue;
            if (id < A.Emax) {
                A.ekey[id] = (unsigned)i * 4u + (unsigned)dir;
                A.val[0][id] = (u64)id << 32;
            }
            ++id;
        }
    } else if (S == 1) {
        if (v.a) A.rec[i] = (u64)before.a << 32 | (u64)before.b;
    } else {
        A.pslot[i] = (int)before.a;
        A.csum[i] = before.b;
    }
}

template <int S> __global__ __launch_bounds__(kThreads) void contour_sum_kernel(ContourArgs A) {
    __shared__ Pair red[kWaves];
    const long n = scan_items<S>(A), base = (long)blockIdx.x * kChunk;
    Pair acc = {0, 0};
    for (int t = 0; t < kItems; ++t) {
        const long i = base + (long)t * kThreads + threadIdx.x;
        if (i < n) acc = acc + scan_value<S>(A, i, n);
    }
    Pair total;
    block_scan(acc, red, total);
    if (threadIdx.x == 0) A.bsum[blockIdx.x] = total;
}

template <int S> __global__ __launch_bounds__(kThreads) void contour_base_kernel(ContourArgs A, int nb) {
    __shared__ Pair red[kWaves];
    Pair carry = {0, 0};
    for (int s = 0; s < nb; s += kThreads) {
        const int j = s + threadIdx.x;
        const Pair v = j < nb ? A.bsum[j] : Pair{0, 0};
        Pair total;
        const Pair before = block_scan(v, red, total);
        if (j < nb) A.bsum[j] = carry + before;
        carry = carry + total;
    }
    if (threadIdx.x == 0) {
        if (S == 0) A.tot[0] = carry.a < A.Emax ? carry.a : A.Emax;
        if (S == 1) A.tot[1] = carry.a;
        if (S == 2) { A.tot[2] = carry.a; A.tot[4] = carry.b; }
    }
}

template <int S> __global__ __launch_bounds__(kThreads) void contour_apply_kernel(ContourArgs A) {
    __shared__ Pair red[kWaves];
    const long n = scan_items<S>(A), base = (long)blockIdx.x * kChunk;
    if (base >= n) return;                              // (the whole workgroup)
    Pair carry = A.bsum[blockIdx.x];
    for (int t = 0; t < kItems; ++t) {
        if (base + (long)t * kThreads >= n) break;      // (the whole workgroup)
        const long i = base + (long)t * kThreads + threadIdx.x;
        const Pair v = i < n ? scan_value<S>(A, i, n) : Pair{0, 0};
        Pair total;
        const Pair before = block_scan(v, red, total);
        if (i < n) scan_emit<S>(A, i, carry + before, v);
        carry = carry + total;
    }
}

// ---- the passes between the scans -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void contour_zero_kernel(ContourArgs A, long words) {
    const long i0 = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i0 < 8) A.tot[i0] = 0;
    if (i0 < kMaxRounds) A.changed[i0] = 0;
    for (long i = i0; i < words; i += (long)gridDim.x * kThreads) A.summary[i] = 0;
}

__global__ __launch_bounds__(kThreads) void contour_link_kernel(ContourArgs A) {
    const long E = A.tot[0];
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < E; i += (long)gridDim.x * kThreads) {
        const Place p = place_of(A, A.ekey[i]);
        const int* lab = A.labels + (long)p.b * A.H * A.W;
        const int k = edge_label(window(A, lab, p.Y, p.X), p.dir);
        const int Y2 = p.Y + (p.dir == 1) - (p.dir == 3), X2 = p.X + (p.dir == 0) - (p.dir == 2);
        if (Y2 < 0 || Y2 > A.H || X2 < 0 || X2 > A.W) continue;        // (an edge never leaves the lattice)
        const Win w2 = window(A, lab, Y2, X2);
        const int m2 = edge_mask(w2);
        const int first = A.conn8 ? 3 : 1;                              // connectivity 8: left, straight, right; 4: right, straight, left
        const int c0 = (p.dir + first) & 3, c1 = p.dir, c2 = (p.dir + 4 - first) & 3;
        int d2 = -1;
        if ((m2 >> c0 & 1) && edge_label(w2, c0) == k) d2 = c0;
        else if ((m2 >> c1 & 1) && edge_label(w2, c1) == k) d2 = c1;
        else if ((m2 >> c2 & 1) && edge_label(w2, c2) == k) d2 = c2;
        if (d2 < 0) continue;                                           // (the label's boundary goes on at every vertex)
        const long s = (long)A.vbase[(long)p.b * A.V1 + (long)Y2 * (A.W + 1) + X2] + __popc((unsigned)(m2 & ((1 << d2) - 1)));
        if ((unsigned long)s >= (unsigned long)E) continue;
        A.prv0[s] = (int)i;
        A.prv[0][s] = (int)i;
    }
}

__global__ __launch_bounds__(kThreads) void contour_jump_kernel(ContourArgs A, int r) {
    if (r > 0 && __hip_atomic_load(A.changed + r - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const long E = A.tot[0];
    const int src = r & 1, dst = src ^ 1;
    const int* ps = A.prv[src];
    const u64* vs = A.val[src];
    const u64 hop = 1ull << r;
    bool any = false;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < E; i += (long)gridDim.x * kThreads) {
        const long p = inside(ps[i], E, i);
        const u64 v = vs[i], w = vs[p] + hop;
        const u64 nv = w < v ? w : v;                   // (w < v only where w names a smaller id: its distance is the larger one)
        A.val[dst][i] = nv;
        A.prv[dst][i] = ps[p];
        any = any || nv != v;
    }
    if (__ballot(any) != 0ull && (threadIdx.x & 63) == 0) atomicOr(A.changed + r, 1);
}

__global__ void contour_rounds_kernel(ContourArgs A) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int ran = 1;                                        // round 0 always runs; round r runs where round r - 1 lowered an id
    for (int r = 0; r + 1 < A.rounds; ++r)
        ran += __hip_atomic_load(A.changed + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ? 1 : 0;
    A.tot[3] = ran;
}

__global__ __launch_bounds__(kThreads) void contour_scatter_kernel(ContourArgs A) {
    const long E = A.tot[0];
    const u64* val = A.val[final_buffer(A)];
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < E; i += (long)gridDim.x * kThreads) {
        const u64 v = val[i];
        const long leader = inside((long)(v >> 32), E, i);
        const long slot = (long)(A.rec[leader] & kLow) + (long)(v & kLow);
        if ((unsigned long)slot < (unsigned long)E) A.perm[slot] = (int)i;
    }
}

// the ring that starts at slot s with the edge e (its leader)
struct Ring { long index; i64 image, label, y, x, points, length, area2; int first_point; };
__device__ __forceinline__ Ring ring_at(const ContourArgs& A, long s, long e, long E, const u64* val) {
    Ring g;
    const Place p = place_of(A, A.ekey[e]);
    g.index = (long)(A.rec[e] >> 32);
    g.image = p.b; g.y = p.Y; g.x = p.X;
    g.label = edge_label(window(A, A.labels + (long)p.b * A.H * A.W, p.Y, p.X), p.dir);
    g.length = (i64)(val[inside(A.prv0[e], E, e)] & kLow) + 1;
    const long end = s + g.length;
    g.first_point = A.pslot[s];
    g.points = (end < E ? (i64)A.pslot[end] : A.tot[2]) - g.first_point;
    g.area2 = (end < E ? A.csum[end] : A.tot[4]) - A.csum[s];
    return g;
}

__device__ __forceinline__ void add64(i64* p, i64 v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

// The rings of one label can be hundreds of thousands (class noise as labels), and four global atomics a ring onto the few rows they
// share serialise at the memory side (measured: 8.4 ms of a 9.5 ms call at 2 x 1024^2).  So a workgroup first sums in LDS: kBins rows
// claimed by compare-and-swap on the row number, 64-bit LDS adds onto them, and one flush of the claimed bins at the end; a ring
// whose bin another row holds goes to memory directly.  All of it integer adds: any order gives the same bits.
constexpr int kBins = 128;

__global__ __launch_bounds__(kThreads) void contour_rings_kernel(ContourArgs A) {
    __shared__ int bin_row[kBins];
    __shared__ u64 bin_sum[kBins][4];
    const long E = A.tot[0];
    const u64* val = A.val[final_buffer(A)];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.totals[0] = A.tot[1]; A.totals[1] = A.tot[2]; A.totals[2] = E > 0 ? A.tot[3] : 0; A.totals[3] = E;
    }
    if ((long)blockIdx.x * kThreads >= E) return;                       // (the whole workgroup: nothing to sum)
    for (int i = threadIdx.x; i < kBins; i += kThreads) {
        bin_row[i] = -1;
        bin_sum[i][0] = bin_sum[i][1] = bin_sum[i][2] = bin_sum[i][3] = 0ull;
    }
    __syncthreads();
    for (long s = (long)blockIdx.x * kThreads + threadIdx.x; s < E; s += (long)gridDim.x * kThreads) {
        const long e = inside(A.perm[s], E, s);
        if ((long)(val[e] >> 32) != e) continue;
        const Ring g = ring_at(A, s, e, E, val);
        if (g.label < 1 || g.label > A.M) continue;
        const int row = (int)(g.image * A.M + (g.label - 1));           // < B * M < 2^26
        const int bin = (int)(((unsigned)row * 2654435761u) >> 25);     // (the top 7 bits: kBins = 128)
        const int held = atomicCAS(&bin_row[bin], -1, row);
        if (held == -1 || held == row) {
            atomicAdd(&bin_sum[bin][0], 1ull); atomicAdd(&bin_sum[bin][1], (u64)g.points);
            atomicAdd(&bin_sum[bin][2], (u64)g.length); atomicAdd(&bin_sum[bin][3], (u64)g.area2);
        } else {
            i64* out = A.summary + (long)row * 4;
            add64(out, 1); add64(out + 1, g.points); add64(out + 2, g.length); add64(out + 3, g.area2);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kThreads) {
        const int row = bin_row[i];
        if (row < 0) continue;
        i64* out = A.summary + (long)row * 4;
        add64(out, (i64)bin_sum[i][0]); add64(out + 1, (i64)bin_sum[i][1]); add64(out + 2, (i64)bin_sum[i][2]); add64(out + 3, (i64)bin_sum[i][3]);
    }
}

__global__ __launch_bounds__(kThreads) void contour_write_kernel(ContourArgs A) {
    const long E = A.tot[0];
    if (A.tot[1] != A.n_rings || A.tot[2] != A.n_points) return;        // not the workspace the caller read its totals from
    const u64* val = A.val[final_buffer(A)];
    if (blockIdx.x == 0 && threadIdx.x == 0) A.ring_offsets[A.n_rings] = (int)A.n_points;
    for (long s = (long)blockIdx.x * kThreads + threadIdx.x; s < E; s += (long)gridDim.x * kThreads) {
        const long e = inside(A.perm[s], E, s);
        const unsigned key = A.ekey[e];
        const int pdir = (int)(A.ekey[inside(A.prv0[e], E, e)] & 3u);
        if (pdir != (int)(key & 3u)) {
            const Place p = place_of(A, key);
            const long slot = A.pslot[s];
            if ((unsigned long)slot < (unsigned long)A.n_points) { A.points[2 * slot] = p.Y; A.points[2 * slot + 1] = p.X; }
        }
        if ((long)(val[e] >> 32) != e) continue;
        const Ring g = ring_at(A, s, e, E, val);
        if ((unsigned long)g.index >= (unsigned long)A.n_rings) continue;
        A.ring_offsets[g.index] = g.first_point;
        i64* row = A.rings + g.index * UAPS_CONTOUR_RING_COLUMNS;
        row[0] = g.image; row[1] = g.label; row[2] = g.y; row[3] = g.x; row[4] = g.points; row[5] = g.length; row[6] = g.area2;
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
struct Layout { size_t head, bsum, vbase, ekey, prv0, prv, val0, val1, perm, pslot, csum, bytes; long V1, V, Emax; int nb; };

int lay_out(int B, int H, int W, int M, Layout& L) {
    if (B <= 0 || H <= 0 || W <= 0 || M < 1) return UAPS_EINVAL;
    if (H > kMaxExtent || W > kMaxExtent || (double)B * H * W * 8.0 >= kTooBig) return UAPS_ERANGE;
    if ((double)B * H * W * 4.0 * 8.0 >= kTooBig || (double)B * M * 32.0 >= kTooBig) return UAPS_ERANGE;    // every array below 2 GiB
    L.V1 = (long)(H + 1) * (W + 1);
    L.V = (long)B * L.V1;                               // <= 4 B H W < 2^28
    L.Emax = 4L * B * H * W;                            // four sides a pixel: < 2^28
    if ((double)L.V * 4.0 >= kTooBig) return UAPS_ERANGE;
    const long most = L.V > L.Emax ? L.V : L.Emax;
    L.nb = (int)((most + kChunk - 1) / kChunk);
    size_t o = 0;
    L.head = o; o += 512;                               // tot[8], then changed[kMaxRounds] from byte 64
    L.bsum = o; o = align256(o + (size_t)L.nb * sizeof(Pair));
    L.vbase = o; o = align256(o + (size_t)L.V * 4);
    L.ekey = o; o = align256(o + (size_t)L.Emax * 4);
    L.prv0 = o; o = align256(o + (size_t)L.Emax * 4);
    L.prv = o; o = align256(o + (size_t)L.Emax * 8);
    L.val0 = o; o = align256(o + (size_t)L.Emax * 8);
    L.val1 = o; o = align256(o + (size_t)L.Emax * 8);
    L.perm = o; o = align256(o + (size_t)L.Emax * 4);
    L.pslot = o; o = align256(o + (size_t)L.Emax * 4);
    L.csum = o; o = align256(o + (size_t)L.Emax * 8);
    L.bytes = o;
    return UAPS_OK;
}

// the checks both entry points share, and the kernels' arguments
int prepare(const uaps_contour_call* call, uaps_contour_call& c, ContourArgs& a, Layout& L) {
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.labels || !c.workspace) return UAPS_EINVAL;
    if (c.connectivity != 4 && c.connectivity != 8) return UAPS_EINVAL;
    const int rc = lay_out(c.B, c.H, c.W, c.max_instances, L);
    if (rc) return rc;
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, L.bytes)) return UAPS_EWORKSPACE;
    memset(&a, 0, sizeof a);
    char* ws = reinterpret_cast<char*>(c.workspace);
    a.B = c.B; a.H = c.H; a.W = c.W; a.M = c.max_instances; a.conn8 = c.connectivity == 8;
    a.V1 = L.V1; a.V = L.V; a.Emax = L.Emax;
    int rounds = 1;                                     // 2^rounds >= the most edges a ring can have, those of one image
    while ((1L << rounds) < 4L * c.H * c.W) ++rounds;   // <= 26
    a.rounds = rounds;
    a.labels = c.labels;
    a.tot = reinterpret_cast<i64*>(ws + L.head);
    a.changed = reinterpret_cast<int*>(ws + L.head + 64);
    a.bsum = reinterpret_cast<Pair*>(ws + L.bsum);
    a.vbase = reinterpret_cast<int*>(ws + L.vbase);
    a.ekey = reinterpret_cast<unsigned*>(ws + L.ekey);
    a.prv0 = reinterpret_cast<int*>(ws + L.prv0);
    a.prv[0] = reinterpret_cast<int*>(ws + L.prv);
    a.prv[1] = a.prv[0] + L.Emax;
    a.rec = reinterpret_cast<u64*>(ws + L.prv);
    a.val[0] = reinterpret_cast<u64*>(ws + L.val0);
    a.val[1] = reinterpret_cast<u64*>(ws + L.val1);
    a.perm = reinterpret_cast<int*>(ws + L.perm);
    a.pslot = reinterpret_cast<int*>(ws + L.pslot);
    a.csum = reinterpret_cast<i64*>(ws + L.csum);
    return UAPS_OK;
}

template <int S> void scan(const ContourArgs& a, long most, hipStream_t st) {
    const int nb = (int)((most + kChunk - 1) / kChunk);
    const dim3 block(kThreads);
    hipLaunchKernelGGL(contour_sum_kernel<S>, dim3(nb), block, 0, st, a);
    hipLaunchKernelGGL(contour_base_kernel<S>, dim3(1), block, 0, st, a, nb);
    hipLaunchKernelGGL(contour_apply_kernel<S>, dim3(nb), block, 0, st, a);
}
}  // namespace

extern "C" int uaps_contours_workspace_bytes(int B, int H, int W, int max_instances, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    Layout L;
    const int rc = lay_out(B, H, W, max_instances, L);
    if (rc) return rc;
    *bytes = L.bytes;
    return UAPS_OK;
}

extern "C" int uaps_contours_trace(const uaps_contour_call* call) {
    uaps_contour_call c;
    ContourArgs a;
    Layout L;
    const int rc = prepare(call, c, a, L);
    if (rc) return rc;
    if (!c.summary || !c.totals || (const void*)c.summary == (const void*)c.labels || (const void*)c.totals == (const void*)c.labels ||
        (const void*)c.totals == (const void*)c.summary)
        return UAPS_EINVAL;
    a.summary = reinterpret_cast<i64*>(c.summary); a.totals = reinterpret_cast<i64*>(c.totals);
    hipStream_t st = (hipStream_t)c.stream;
    const long rows = (long)c.B * c.max_instances;
    uaps::account_bytes((double)c.B * c.H * c.W * 4.0 + 32.0 * (double)rows);
    const dim3 block(kThreads);
    const dim3 edges(grid_for(L.Emax, kMaxGrid));
    hipLaunchKernelGGL(contour_zero_kernel, dim3(grid_for(rows * 4, kMaxGrid)), block, 0, st, a, rows * 4);
    scan<0>(a, L.V, st);
    hipLaunchKernelGGL(contour_link_kernel, edges, block, 0, st, a);
    for (int r = 0; r < a.rounds; ++r) UAPS_LAUNCH_MAIN(contour_jump_kernel, edges, block, 0, st, a, r);
    hipLaunchKernelGGL(contour_rounds_kernel, dim3(1), dim3(64), 0, st, a);
    scan<1>(a, L.Emax, st);
    hipLaunchKernelGGL(contour_scatter_kernel, edges, block, 0, st, a);
    scan<2>(a, L.Emax, st);
    hipLaunchKernelGGL(contour_rings_kernel, edges, block, 0, st, a);
    return (int)hipGetLastError();
}

extern "C" int uaps_contours_write(const uaps_contour_call* call) {
    uaps_contour_call c;
    ContourArgs a;
    Layout L;
    const int rc = prepare(call, c, a, L);
    if (rc) return rc;
    if (!c.points || !c.ring_offsets || !c.rings) return UAPS_EINVAL;
    if (c.n_rings < 1 || c.n_points < 4 || c.n_rings >= 2147483648LL || c.n_points >= 2147483648LL) return UAPS_EINVAL;
    if (c.ring_capacity < c.n_rings || c.point_capacity < c.n_points) return UAPS_EINVAL;      // outputs too small for the totals
    a.n_rings = c.n_rings; a.n_points = c.n_points;
    a.points = c.points; a.ring_offsets = c.ring_offsets; a.rings = reinterpret_cast<i64*>(c.rings);
    hipStream_t st = (hipStream_t)c.stream;
    uaps::account_bytes(8.0 * (double)c.n_points + 4.0 * (double)(c.n_rings + 1) + 8.0 * UAPS_CONTOUR_RING_COLUMNS * (double)c.n_rings);
    UAPS_LAUNCH_MAIN(contour_write_kernel, dim3(grid_for(L.Emax, kMaxGrid)), dim3(kThreads), 0, st, a);
    return (int)hipGetLastError();
}
