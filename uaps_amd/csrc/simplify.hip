// Contour simplification for gfx950 (include/uaps_hip.h, uaps_contours_simplify_mark / uaps_contours_simplify_write): exact
// Ramer-Douglas-Peucker on the rings of uaps_contours_write.  A ring of n points p_0 .. p_{n-1} (index n is p_0 again) keeps p_0, the
// point b farthest from p_0, and inside every interval (i, j) of kept points the interior point with the largest deviation from the
// SEGMENT p_i -> p_j while that deviation exceeds the tolerance; the deviation is the fraction num / den of squared pixels of
// deviation() below, "exceeds" is 256 num > e16^2 den, and every tie goes to the lowest index.  If neither (0, b) nor (b, n) splits,
// the point with the largest num of both is kept all the same (never below a triangle) and the rule goes on inside its two halves.
//
// The depth of the recursion is linear in n at worst (a comb of rising teeth peels one tooth a round), so the rounds run INSIDE the
// kernel, one ring to a wave or a workgroup, until a round splits no interval.  A point's whole state is (lo, hi), the kept points
// that bracket it; a round is: every point of an open interval posts its num to the slot of its lo, the slot's arg-max k is read
// back, the points left of k take hi = k, those right of it lo = k, k is kept; an interval whose arg-max does not exceed the
// tolerance closes and its points skip the arithmetic from then on.  Three forms, by the ring's point count:
//   simplify_wave_kernel          n <= wave_max (64 at most): a ring to a wave, a point to a lane, the rings strided over a fixed grid.
//                                 State in registers, bracket points by shuffles, the per-interval arg-max a segmented suffix-max
//                                 of the key  num << 12 | (4095 - index)  over the lanes; no barrier, no LDS.
//   simplify_block_kernel<true, 256>    n <= lds_max (2048 at most): a ring to a workgroup; packed points (13 + 13 bits), lo, hi and one
//                                 64-bit key slot a point in LDS (32 KiB); one LDS max-atomic of the same key a point and round.
//   simplify_block_kernel<false, 1024>  any n: a ring to a workgroup of 1024 threads strided over it, state in the workspace, the arg-max as two integer
//                                 atomics (max of num, then min of the index among the equal).
// The rings of the two workgroup forms are gathered into index lists first (simplify_classify_kernel) and a fixed grid walks each
// list, so a map of hundreds of thousands of four-point rings launches no idle workgroup a ring.  Every form ends a ring the same
// way: the kept count, the rank of every kept point inside the ring, the shoelace sum of the simplified ring, and kept - n added to
// the `points` column of the summary copy.  simplify_sum / _base / _apply scan the kept counts into the new ring offsets, and
// simplify_write_kernel, after the host has read the total, stores every kept point at its ring's base plus its rank.
// Integers only, no float, no scratch; only integer max / min / add atomics, so every form and every run gives the same bits.
#include "call_common.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256; using uaps::u64;
typedef long long i64;

constexpr int kWaveCap = UAPS_SIMPLIFY_WAVE_MAX, kLdsCap = UAPS_SIMPLIFY_LDS_MAX;
constexpr int kMaxE16 = UAPS_SIMPLIFY_MAX_E16;
constexpr int kGlobalThreads = 1024;
constexpr int kWaveGrid = 2048, kLdsGrid = 1024, kGlobalGrid = 512, kFlatGrid = 2048;
constexpr int kItems = 16, kChunk = kThreads * kItems;          // rings of one workgroup of the scan
constexpr int kKept = -1, kDone = -2, kNew = -3;                // lo of a point that is no member of an open interval
// the bounds of the arithmetic: coordinates in 0 .. 4096, so |P - A|^2, |d|^2 and |cross| stay within 2^25, num within 2^50, and both
// sides of 256 num > e16^2 den, like the 62-bit key, inside a signed 64-bit integer
static_assert(2LL * UAPS_CONTOUR_MAX_EXTENT * UAPS_CONTOUR_MAX_EXTENT == 1LL << 25, "squared lengths within 2^25");
static_assert(kLdsCap <= 4096 && kWaveCap == 64 && 50 + 12 < 64, "the key holds num << 12 | 12 bits of index");
static_assert((i64)kMaxE16 * kMaxE16 == 1LL << 20 && 20 + 25 < 63 && 8 + 50 < 63, "the comparison stays inside int64");
static_assert(kLdsCap * 16 <= 48 * 1024, "the LDS form's state");

struct SimplifyArgs {
    long N, L, rows;                    // points, rings, rows of the summary
    int M, wave_max, lds_max;
    i64 tol;                            // e16^2
    const int* points;                  // [N][2], (y, x)
    const int* offsets;                 // [L + 1]
    const i64* rings;                   // [L][7]
    const i64* summary_in;
    i64* summary_out;                   // [rows][4]
    i64* totals;                        // the caller's [4]
    i64* head;                          // [0] L  [1] kept points  [2] rings of the LDS list  [3] rings of the global list
    i64* bsum;                          // the scan's block sums
    int* kept;                          // [L]: kept points of a ring
    i64* area;                          // [L]: the shoelace sum of the simplified ring
    int* noff;                          // [L]: the ring's first slot in the output
    int* list[2];                       // [L] each: the rings of the LDS and of the global form
    int* pring;                         // [N]: the ring of a point
    int* slot;                          // [N]: the rank of a kept point inside its ring, -1 for a dropped one
    int* glo;                           // [N] each: the global form's lo, hi, and at a kept point the slot of the interval it opens
    int* ghi;
    u64* gmax;
    unsigned* gidx;
    i64 n_rings, n_points_out, point_capacity, ring_capacity;      // write
    int* points_out;
    int* offsets_out;
    i64* rings_out;
    i64* stats;
};

struct Span { long o0; int n; };
// the points of ring r; anything that does not lie inside [0, N] is an empty ring and touches nothing
__device__ __forceinline__ Span span_of(const SimplifyArgs& A, long r) {
    const long a = A.offsets[r], b = A.offsets[r + 1];
    Span s = {a, 0};
    if (a >= 0 && b > a && b <= A.N) s.n = (int)(b - a);
    return s;
}

struct Dev { i64 num, den; };
// the deviation of P from the segment A -> B
__device__ __forceinline__ Dev deviation(int py, int px, int ay, int ax, int by, int bx) {
    const i64 dy = by - ay, dx = bx - ax, qy = py - ay, qx = px - ax;
    const i64 L2 = dy * dy + dx * dx, t = qy * dy + qx * dx, q2 = qy * qy + qx * qx;
    if (L2 == 0) return Dev{q2, 1};
    if (t <= 0) return Dev{q2 * L2, L2};
    if (t >= L2) {
        const i64 ry = py - by, rx = px - bx;
        return Dev{(ry * ry + rx * rx) * L2, L2};
    }
    const i64 c = dx * qy - dy * qx;
    return Dev{c * c, L2};
}

__device__ __forceinline__ bool exceeds(i64 num, i64 den, i64 tol) { return 256 * num > tol * den; }
__device__ __forceinline__ void add64(i64* p, i64 v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

// what every form stores for a finished ring
__device__ __forceinline__ void finish_ring(const SimplifyArgs& A, long r, int n, int kept, i64 area2) {
    A.kept[r] = kept;
    A.area[r] = area2;
    if (kept == n) return;
    const i64 image = A.rings[r * UAPS_CONTOUR_RING_COLUMNS], label = A.rings[r * UAPS_CONTOUR_RING_COLUMNS + 1];
    if (image < 0 || image >= A.rows || label < 1 || label > A.M) return;
    const i64 row = image * A.M + (label - 1);
    if (row < A.rows) add64(A.summary_out + row * UAPS_CONTOUR_COLUMNS + 1, (i64)kept - n);
}

// ---- the passes in front of the rings -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void simplify_copy_kernel(SimplifyArgs A) {
    const long i0 = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i0 < 4) A.head[i0] = 0;
    for (long i = i0; i < A.rows * UAPS_CONTOUR_COLUMNS; i += (long)gridDim.x * kThreads) A.summary_out[i] = A.summary_in[i];
}

__global__ __launch_bounds__(kThreads) void simplify_classify_kernel(SimplifyArgs A) {
    for (long r = (long)blockIdx.x * kThreads + threadIdx.x; r < A.L; r += (long)gridDim.x * kThreads) {
        const int n = span_of(A, r).n;
        if (n == 0) { A.kept[r] = 0; A.area[r] = 0; continue; }
        if (n <= A.wave_max) continue;
        const int which = n <= A.lds_max ? 0 : 1;
        const u64 at = atomicAdd(reinterpret_cast<u64*>(A.head + 2 + which), 1ull);
        if (at < (u64)A.L) A.list[which][at] = (int)r;
    }
}

// ---- the wave form ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

__device__ __forceinline__ i64 wave_sum_i64(i64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kThreads) void simplify_wave_kernel(SimplifyArgs A) {
    const int lane = threadIdx.x & 63;
    const long waves = (long)gridDim.x * kWaves;
    for (long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); r < A.L; r += waves) {
        const Span s = span_of(A, r);                                   // (the same in every lane of the wave)
        const int n = s.n;
        if (n == 0 || n > A.wave_max || n > 64) continue;
        const bool in = lane < n;
        const int y = in ? A.points[2 * (s.o0 + lane)] : 0, x = in ? A.points[2 * (s.o0 + lane) + 1] : 0;
        // anchor b: the point farthest from p_0, the lowest index among the equal
        const i64 ey = y - __shfl(y, 0, 64), ex = x - __shfl(x, 0, 64);
        const u64 far = wave_max_u64(in && lane > 0 ? (u64)(ey * ey + ex * ex) << 12 | (u64)(4095 - lane) : 0ull);
        const int b = far ? 4095 - (int)(far & 4095u) : 0;
        bool kept = in && (lane == 0 || lane == b), done = n < 3;
        int lo = lane < b ? 0 : b, hi = lane < b ? b : n;
        for (int round = 0; round < 64; ++round) {
            const bool active = in && !kept && !done;
            const int hi0 = hi == n ? 0 : hi;
            const int ay = __shfl(y, lo, 64), ax = __shfl(x, lo, 64), by = __shfl(y, hi0, 64), bx = __shfl(x, hi0, 64);
            const Dev d = deviation(y, x, ay, ax, by, bx);
            u64 key = active ? (u64)d.num << 12 | (u64)(4095 - lane) : 0ull;
            const int seg = in && !kept ? lo : 64 + lane;               // the lanes of one interval are consecutive
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 ok = __shfl_down(key, o, 64);
                const int os = __shfl_down(seg, o, 64);
                if (lane + o < 64 && os == seg && ok > key) key = ok;
            }
            const u64 K = __shfl(key, (lo + 1) & 63, 64);               // the suffix-max at the interval's first lane
            bool split = exceeds((i64)(K >> 12), d.den, A.tol);
            if (round == 0) {                                           // never below a triangle
                const u64 K0 = __shfl(key, 1, 64), Kt = __shfl(key, (b + 1) & 63, 64), Kb = b + 1 < n ? Kt : 0ull;
                const bool none = !exceeds((i64)(K0 >> 12), d.den, A.tol) && !exceeds((i64)(Kb >> 12), d.den, A.tol);
                const u64 Kf = K0 > Kb ? K0 : Kb;
                if (none && K == Kf && (Kf >> 12) != 0) split = true;
            }
            if (active) {
                const int k = 4095 - (int)(K & 4095u);
                if (!split) done = true;
                else if (lane == k) kept = true;
                else if (lane < k) hi = k;
                else lo = k;
            }
            if (!__any(active && split)) break;
        }
        const u64 mask = __ballot(kept);
        const int count = __popcll(mask);
        const u64 above = lane < 63 ? mask & ~((2ull << lane) - 1ull) : 0ull;
        const int nxt = above ? __ffsll((long long)above) - 1 : 0;
        const int ny = __shfl(y, nxt, 64), nx = __shfl(x, nxt, 64);
        const i64 area2 = wave_sum_i64(kept ? (i64)x * ny - (i64)nx * y : 0);
        if (in) {
            A.pring[s.o0 + lane] = (int)r;
            A.slot[s.o0 + lane] = kept ? __popcll(mask & ((1ull << lane) - 1ull)) : -1;
        }
        if (lane == 0) finish_ring(A, r, n, count, area2);
    }
}

// ---- the workgroup forms ------------------------------------------------------------------------------------------------------------
// where a ring's state lives: LDS (points packed, 16-bit brackets, one key slot) or the workspace (two words a slot)
struct LdsState {
    unsigned* pt; short* lo; short* hi; u64* key;
    __device__ __forceinline__ void load(const SimplifyArgs& A, long o0, int i) {
        pt[i] = ((unsigned)A.points[2 * (o0 + i)] & 8191u) << 13 | ((unsigned)A.points[2 * (o0 + i) + 1] & 8191u);
    }
    __device__ __forceinline__ int y(int i) const { return (int)(pt[i] >> 13); }
    __device__ __forceinline__ int x(int i) const { return (int)(pt[i] & 8191u); }
    __device__ __forceinline__ int get_lo(int i) const { return lo[i]; }
    __device__ __forceinline__ int get_hi(int i) const { return hi[i]; }
    __device__ __forceinline__ void set_lo(int i, int v) { lo[i] = (short)v; }
    __device__ __forceinline__ void set_hi(int i, int v) { hi[i] = (short)v; }
    __device__ __forceinline__ void clear(int s) { key[s] = 0ull; }
    __device__ __forceinline__ void post(int s, i64 num, int i) { atomicMax(&key[s], (u64)num << 12 | (u64)(4095 - i)); }
    __device__ __forceinline__ void post_index(int, i64, int) {}
    __device__ __forceinline__ i64 best(int s, int& k) const { const u64 K = key[s]; k = 4095 - (int)(K & 4095u); return (i64)(K >> 12); }
};

struct GlobalState {
    const int* p; int* lo; int* hi; u64* mx; unsigned* idx;            // all of them at the ring's first point
    __device__ __forceinline__ void load(const SimplifyArgs&, long, int) {}
    __device__ __forceinline__ int y(int i) const { return p[2 * (long)i]; }
    __device__ __forceinline__ int x(int i) const { return p[2 * (long)i + 1]; }
    __device__ __forceinline__ int get_lo(int i) const { return lo[i]; }
    __device__ __forceinline__ int get_hi(int i) const { return hi[i]; }
    __device__ __forceinline__ void set_lo(int i, int v) { lo[i] = v; }
    __device__ __forceinline__ void set_hi(int i, int v) { hi[i] = v; }
    __device__ __forceinline__ void clear(int s) { mx[s] = 0ull; idx[s] = 0xffffffffu; }
    __device__ __forceinline__ void post(int s, i64 num, int) { atomicMax(&mx[s], (u64)num); }
    // (what the atomics of other lanes left is read at agent scope: past the vector cache, as the atomics went)
    __device__ __forceinline__ u64 top(int s) const { return __hip_atomic_load(mx + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void post_index(int s, i64 num, int i) { if ((u64)num == top(s)) atomicMin(&idx[s], (unsigned)i); }
    __device__ __forceinline__ i64 best(int s, int& k) const {
        k = (int)__hip_atomic_load(idx + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (i64)top(s);
    }
};

// what point i posts in a round: its squared distance from p_0 while the anchor is sought, its deviation afterwards
template <typename S> __device__ __forceinline__ Dev value_of(const S& st, int i, int lo, int hi, int n, bool anchor) {
    if (anchor) {
        const i64 ey = st.y(i) - st.y(0), ex = st.x(i) - st.x(0);
        return Dev{ey * ey + ex * ex, 1};
    }
    const int h = hi == n ? 0 : hi;
    return deviation(st.y(i), st.x(i), st.y(lo), st.x(lo), st.y(h), st.x(h));
}

template <bool kLds, int kT, typename S> __device__ __forceinline__ void simplify_ring(const SimplifyArgs& A, S& st, long r, const Span s, int* wsum, i64* asum) {
    const int n = s.n, tid = threadIdx.x;
    for (int i = tid; i < n; i += kT) {
        st.load(A, s.o0, i);
        st.set_lo(i, i == 0 ? kKept : 0);
        st.set_hi(i, n);
        st.clear(i);
    }
    __syncthreads();
    int b = 0;                                                          // the anchor, once it is known
    // round 0 seeks the anchor, round 1 is the top level with its triangle rule; a ring of n points is done after n rounds at the most
    for (int round = 0; round < n + 2; ++round) {
        const bool anchor = round == 0;
        for (int i = tid; i < n; i += kT) {
            const int lo = st.get_lo(i);
            if (lo < 0) continue;
            st.post(lo, value_of(st, i, lo, st.get_hi(i), n, anchor).num, i);
        }
        __syncthreads();
        if (!kLds) {
            for (int i = tid; i < n; i += kT) {
                const int lo = st.get_lo(i);
                if (lo < 0) continue;
                st.post_index(lo, value_of(st, i, lo, st.get_hi(i), n, anchor).num, i);
            }
            __syncthreads();
        }
        int forced = -1;                                                // the slot whose arg-max the triangle rule keeps
        if (round == 1) {
            int k0, kb;
            const i64 m0 = st.best(0, k0), mb = st.best(b, kb);
            const i64 dy = st.y(b) - st.y(0), dx = st.x(b) - st.x(0), den = dy * dy + dx * dx;      // (of both: the segment p_0 <-> p_b)
            if (!exceeds(m0, den, A.tol) && !exceeds(mb, den, A.tol) && (m0 > 0 || mb > 0))
                forced = m0 > mb || (m0 == mb && k0 < kb) ? 0 : b;
        }
        bool split = false;
        for (int i = tid; i < n; i += kT) {
            const int lo = st.get_lo(i);
            if (lo < 0) continue;
            const int hi = st.get_hi(i);
            int k;
            const i64 m = st.best(lo, k);
            const bool cut = anchor ? m > 0 : (lo == forced || exceeds(m, value_of(st, i, lo, hi, n, false).den, A.tol));
            if (!cut || k < 0 || k >= n) { st.set_lo(i, kDone); continue; }
            split = true;
            if (i == k) { st.set_lo(i, kNew); st.set_hi(i, lo); }       // (hi of a kept point: the slot it was posted to)
            else if (i < k) st.set_hi(i, k);
            else st.set_lo(i, k);
        }
        if (anchor) {                                                   // (before the slots are cleared: every thread reads the anchor)
            int k;
            b = st.best(0, k) > 0 && k > 0 && k < n ? k : 0;
        }
        if (!__syncthreads_or(split)) break;
        for (int i = tid; i < n; i += kT) {
            if (st.get_lo(i) != kNew) continue;
            st.clear(i);
            st.clear(st.get_hi(i));
            st.set_lo(i, kKept);
        }
        __syncthreads();
        if (b == 0) break;                                              // (every point on p_0: nothing to split)
    }
    // the kept count, the ranks and the shoelace sum of the kept points
    const int lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    i64 area2 = 0;
    for (int base = 0; base < n; base += kT) {
        const int i = base + tid;
        const bool kept = i < n && st.get_lo(i) == kKept;
        const u64 mask = __ballot(kept);
        if (lane == 0) wsum[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kT / 64; ++w) { before += w < wave ? wsum[w] : 0; total += wsum[w]; }
        if (i < n) {
            A.pring[s.o0 + i] = (int)r;
            A.slot[s.o0 + i] = kept ? carry + before + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
        }
        if (kept) {
            const int j = i + 1;
            int nxt = j >= n ? 0 : (st.get_lo(j) == kKept ? j : st.get_hi(j));
            if (nxt < 0 || nxt >= n) nxt = 0;
            area2 += (i64)st.x(i) * st.y(nxt) - (i64)st.x(nxt) * st.y(i);
        }
        carry += total;
        __syncthreads();
    }
    area2 = wave_sum_i64(area2);
    if (tid == 0) *asum = 0;
    __syncthreads();
    if (lane == 0) add64(asum, area2);
    __syncthreads();
    if (tid == 0) finish_ring(A, r, n, carry, *asum);
    __syncthreads();
}

// (the LDS form: kThreads threads for its 2048 points at the most; the global form: 1024, a quarter of the trips round a long ring)
template <bool kLds, int kT> __global__ __launch_bounds__(kT) void simplify_block_kernel(SimplifyArgs A) {
    __shared__ unsigned s_pt[kLds ? kLdsCap : 1];
    __shared__ short s_lo[kLds ? kLdsCap : 1], s_hi[kLds ? kLdsCap : 1];
    __shared__ u64 s_key[kLds ? kLdsCap : 1];
    __shared__ int wsum[kT / 64];
    __shared__ i64 asum;
    const int which = kLds ? 0 : 1;
    i64 count = A.head[2 + which];
    if (count > A.L) count = A.L;
    for (long j = blockIdx.x; j < count; j += gridDim.x) {
        const long r = A.list[which][j];
        if ((unsigned long)r >= (unsigned long)A.L) continue;           // (the whole workgroup)
        const Span s = span_of(A, r);
        if (s.n == 0 || (kLds && s.n > kLdsCap)) continue;
        if (kLds) {
            LdsState st = {s_pt, s_lo, s_hi, s_key};
            simplify_ring<true, kT>(A, st, r, s, wsum, &asum);
        } else {
            GlobalState st = {A.points + 2 * s.o0, A.glo + s.o0, A.ghi + s.o0, A.gmax + s.o0, A.gidx + s.o0};
            simplify_ring<false, kT>(A, st, r, s, wsum, &asum);
        }
    }
}

// ---- the scan of the kept counts ------------------------------------------------------------------------------------------------------
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

__global__ __launch_bounds__(kThreads) void simplify_sum_kernel(SimplifyArgs A) {
    __shared__ i64 red[kWaves];
    const long base = (long)blockIdx.x * kChunk;
    i64 acc = 0;
    for (int t = 0; t < kItems; ++t) {
        const long r = base + (long)t * kThreads + threadIdx.x;
        if (r < A.L) acc += A.kept[r];
    }
    i64 total;
    block_scan(acc, red, total);
    if (threadIdx.x == 0) A.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void simplify_base_kernel(SimplifyArgs A, int nb) {
    __shared__ i64 red[kWaves];
    i64 carry = 0;
    for (int s = 0; s < nb; s += kThreads) {
        const int j = s + threadIdx.x;
        const i64 v = j < nb ? A.bsum[j] : 0;
        i64 total;
        const i64 before = block_scan(v, red, total);
        if (j < nb) A.bsum[j] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        A.head[0] = A.L; A.head[1] = carry;
        A.totals[0] = A.L; A.totals[1] = carry; A.totals[2] = A.head[2]; A.totals[3] = A.head[3];
    }
}

__global__ __launch_bounds__(kThreads) void simplify_apply_kernel(SimplifyArgs A) {
    __shared__ i64 red[kWaves];
    const long base = (long)blockIdx.x * kChunk;
    i64 carry = A.bsum[blockIdx.x];
    for (int t = 0; t < kItems; ++t) {
        if (base + (long)t * kThreads >= A.L) break;    // (the whole workgroup)
        const long r = base + (long)t * kThreads + threadIdx.x;
        const i64 v = r < A.L ? A.kept[r] : 0;
        i64 total;
        const i64 before = block_scan(v, red, total);
        if (r < A.L) A.noff[r] = (int)(carry + before);
        carry += total;
    }
}

__global__ __launch_bounds__(kThreads) void simplify_write_kernel(SimplifyArgs A) {
    if (A.head[0] != A.n_rings || A.head[1] != A.n_points_out) return;  // not the workspace the caller read its total from
    const long i0 = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    if (i0 == 0) A.offsets_out[A.L] = (int)A.n_points_out;
    for (long i = i0; i < A.N; i += step) {
        const long rank = A.slot[i], r = A.pring[i];
        if (rank < 0 || (unsigned long)r >= (unsigned long)A.L) continue;
        const long at = (long)A.noff[r] + rank;
        if ((unsigned long)at >= (unsigned long)A.n_points_out) continue;
        A.points_out[2 * at] = A.points[2 * i];
        A.points_out[2 * at + 1] = A.points[2 * i + 1];
    }
    for (long r = i0; r < A.L; r += step) {
        A.offsets_out[r] = A.noff[r];
        const i64* src = A.rings + r * UAPS_CONTOUR_RING_COLUMNS;
        i64* row = A.rings_out + r * UAPS_CONTOUR_RING_COLUMNS;
        for (int c = 0; c < UAPS_CONTOUR_RING_COLUMNS; ++c) row[c] = c == 4 ? (i64)A.kept[r] : src[c];
        A.stats[2 * r] = span_of(A, r).n;
        A.stats[2 * r + 1] = A.area[r];
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
struct Layout { size_t head, bsum, kept, area, noff, list0, list1, pring, slot, glo, ghi, gmax, gidx, bytes; int nb; };

int lay_out(i64 n_points, i64 n_rings, Layout& L) {
    if (n_points < 1 || n_rings < 1) return UAPS_EINVAL;
    if (n_points >= 1073741824LL || n_rings > n_points) return UAPS_ERANGE;     // (2 * n_points indexes the coordinates)
    const size_t N = (size_t)n_points, R = (size_t)n_rings;
    L.nb = (int)((n_rings + kChunk - 1) / kChunk);
    size_t o = 0;
    L.head = o; o += 256;
    L.bsum = o; o = align256(o + (size_t)L.nb * 8);
    L.kept = o; o = align256(o + R * 4);
    L.area = o; o = align256(o + R * 8);
    L.noff = o; o = align256(o + R * 4);
    L.list0 = o; o = align256(o + R * 4);
    L.list1 = o; o = align256(o + R * 4);
    L.pring = o; o = align256(o + N * 4);
    L.slot = o; o = align256(o + N * 4);
    L.glo = o; o = align256(o + N * 4);
    L.ghi = o; o = align256(o + N * 4);
    L.gmax = o; o = align256(o + N * 8);
    L.gidx = o; o = align256(o + N * 4);
    L.bytes = o;
    return UAPS_OK;
}

// the checks both entry points share, and the kernels' arguments
int prepare(const uaps_simplify_call* call, uaps_simplify_call& c, SimplifyArgs& a, Layout& L) {
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.points || !c.ring_offsets || !c.rings || !c.workspace) return UAPS_EINVAL;
    if (c.B < 1 || c.max_instances < 1 || c.e16 < 0 || c.e16 > kMaxE16) return UAPS_EINVAL;
    if (c.wave_max > kWaveCap || c.lds_max > kLdsCap || c.wave_max < UAPS_SIMPLIFY_OFF || c.lds_max < UAPS_SIMPLIFY_OFF) return UAPS_EINVAL;
    if ((double)c.B * c.max_instances * 32.0 >= kTooBig) return UAPS_ERANGE;
    const int rc = lay_out(c.n_points, c.n_rings, L);
    if (rc) return rc;
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, L.bytes)) return UAPS_EWORKSPACE;
    memset(&a, 0, sizeof a);
    char* ws = reinterpret_cast<char*>(c.workspace);
    a.N = (long)c.n_points; a.L = (long)c.n_rings; a.rows = (long)c.B * c.max_instances; a.M = c.max_instances;
    a.wave_max = c.wave_max == 0 ? kWaveCap : c.wave_max;               // (UAPS_SIMPLIFY_OFF: below every ring's point count)
    a.lds_max = c.lds_max == 0 ? kLdsCap : c.lds_max;
    a.tol = (i64)c.e16 * c.e16;
    a.points = c.points; a.offsets = c.ring_offsets; a.rings = reinterpret_cast<const i64*>(c.rings);
    a.head = reinterpret_cast<i64*>(ws + L.head);
    a.bsum = reinterpret_cast<i64*>(ws + L.bsum);
    a.kept = reinterpret_cast<int*>(ws + L.kept);
    a.area = reinterpret_cast<i64*>(ws + L.area);
    a.noff = reinterpret_cast<int*>(ws + L.noff);
    a.list[0] = reinterpret_cast<int*>(ws + L.list0);
    a.list[1] = reinterpret_cast<int*>(ws + L.list1);
    a.pring = reinterpret_cast<int*>(ws + L.pring);
    a.slot = reinterpret_cast<int*>(ws + L.slot);
    a.glo = reinterpret_cast<int*>(ws + L.glo);
    a.ghi = reinterpret_cast<int*>(ws + L.ghi);
    a.gmax = reinterpret_cast<u64*>(ws + L.gmax);
    a.gidx = reinterpret_cast<unsigned*>(ws + L.gidx);
    return UAPS_OK;
}
}  // namespace

extern "C" int uaps_contours_simplify_workspace_bytes(int64_t n_points, int64_t n_rings, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    Layout L;
    const int rc = lay_out(n_points, n_rings, L);
    if (rc) return rc;
    *bytes = L.bytes;
    return UAPS_OK;
}

extern "C" int uaps_contours_simplify_mark(const uaps_simplify_call* call) {
    uaps_simplify_call c;
    SimplifyArgs a;
    Layout L;
    const int rc = prepare(call, c, a, L);
    if (rc) return rc;
    if (!c.summary_in || !c.summary_out || !c.totals || (const void*)c.summary_in == (const void*)c.summary_out ||
        (const void*)c.totals == (const void*)c.summary_out || (const void*)c.totals == (const void*)c.summary_in)
        return UAPS_EINVAL;
    a.summary_in = reinterpret_cast<const i64*>(c.summary_in); a.summary_out = reinterpret_cast<i64*>(c.summary_out);
    a.totals = reinterpret_cast<i64*>(c.totals);
    hipStream_t st = (hipStream_t)c.stream;
    uaps::account_bytes(8.0 * (double)a.N + 4.0 * (double)(a.L + 1) + 16.0 * (double)a.L + 64.0 * (double)a.rows);
    const dim3 block(kThreads);
    const int rings_grid = grid_for(a.L, kFlatGrid);
    hipLaunchKernelGGL(simplify_copy_kernel, dim3(grid_for(a.rows * UAPS_CONTOUR_COLUMNS, kFlatGrid)), block, 0, st, a);
    hipLaunchKernelGGL(simplify_classify_kernel, dim3(rings_grid), block, 0, st, a);
    if (a.wave_max >= 1)
        UAPS_LAUNCH_MAIN(simplify_wave_kernel, dim3((int)((a.L + kWaves - 1) / kWaves < kWaveGrid ? (a.L + kWaves - 1) / kWaves : kWaveGrid)), block, 0, st, a);
    hipLaunchKernelGGL((simplify_block_kernel<true, kThreads>), dim3((int)(a.L < kLdsGrid ? a.L : kLdsGrid)), block, 0, st, a);
    hipLaunchKernelGGL((simplify_block_kernel<false, kGlobalThreads>), dim3((int)(a.L < kGlobalGrid ? a.L : kGlobalGrid)), dim3(kGlobalThreads), 0, st, a);
    hipLaunchKernelGGL(simplify_sum_kernel, dim3(L.nb), block, 0, st, a);
    hipLaunchKernelGGL(simplify_base_kernel, dim3(1), block, 0, st, a, L.nb);
    hipLaunchKernelGGL(simplify_apply_kernel, dim3(L.nb), block, 0, st, a);
    return (int)hipGetLastError();
}

extern "C" int uaps_contours_simplify_write(const uaps_simplify_call* call) {
    uaps_simplify_call c;
    SimplifyArgs a;
    Layout L;
    const int rc = prepare(call, c, a, L);
    if (rc) return rc;
    if (!c.points_out || !c.ring_offsets_out || !c.rings_out || !c.ring_stats) return UAPS_EINVAL;
    if (c.n_points_out < 1 || c.n_points_out > c.n_points) return UAPS_EINVAL;
    if (c.ring_capacity < c.n_rings || c.point_capacity < c.n_points_out) return UAPS_EINVAL;    // outputs too small for the totals
    a.n_rings = c.n_rings; a.n_points_out = c.n_points_out; a.point_capacity = c.point_capacity; a.ring_capacity = c.ring_capacity;
    a.points_out = c.points_out; a.offsets_out = c.ring_offsets_out;
    a.rings_out = reinterpret_cast<i64*>(c.rings_out); a.stats = reinterpret_cast<i64*>(c.ring_stats);
    hipStream_t st = (hipStream_t)c.stream;
    uaps::account_bytes(8.0 * (double)a.N + 8.0 * (double)c.n_points_out + (4.0 + 16.0 + 16.0 * UAPS_CONTOUR_RING_COLUMNS) * (double)a.L);
    UAPS_LAUNCH_MAIN(simplify_write_kernel, dim3(grid_for(a.N, kFlatGrid)), dim3(kThreads), 0, st, a);
    return (int)hipGetLastError();
}
