// Defect instance extraction and run-length masks for gfx950 (include/uaps_hip.h, uaps_label_instances / uaps_rle_*).
//
// uaps_label_instances: connected components of a class mask [B,H,W] (int64), numbered per image by their first pixel in raster
// order, with a compact per-component table.  Seven launches, every one a coherence point for the next; inside a launch no workgroup
// ever waits for another (no flags, no spin loops): every union loop ends by the monotone decrease of the parent words alone.
//   1 tile_label_kernel    a 16 x 16 tile in LDS: union-find with atomicMin over the backward neighbours of every pixel, then every
//                          pixel's parent := the image-local index of its tile-local root (the smallest raster index of the tile-local
//                          component; tile-local raster order and image raster order agree inside a tile).  Plain stores; the area
//                          scratch word of every pixel is zeroed on the way.
//   2 seam_merge_kernel    one lane per seam pixel (first row / first column of a tile) and its up to three neighbours across the seam
//                          (only the joins the tile pass does not already imply: cc_common.hpp).
//                          Every parent word is read with relaxed agent-scope atomic loads and lowered with atomicMin.  A stale read is
//                          an older parent, still an ancestor in the same component, so it costs iterations, never correctness.
//   3 flatten_area_kernel  parent -> root (the component's smallest pixel index = its first pixel), stored into `labels`; integer
//                          atomicAdds onto the roots' area words: the lanes of a 64-pixel group's leading root are counted by ballot
//                          and carried on by the wave over its 16 groups, the other roots send one add per run of equal roots.
//   4 chunk_count_kernel / scan_segments_kernel / number_roots_kernel
//                          "is a root and area >= min_area" counted per 256-pixel raster chunk, the chunk counts scanned per image
//                          (count[b] = the total), the surviving roots numbered 1..N_b in raster order; the root's lane writes the
//                          row's class, area, y0, first pixel and the neutral elements of the box.
//   5 final_kernel         labels := number of the pixel's root; per run of equal numbers inside a wave and a row one atomicMin /
//                          atomicMax on the box and one 64-bit integer atomicAdd per map: sums of
//                          q(v) = (int64) rintf(clamp(v, -65536, 65536) * 2^24), NaN -> 0.  Integer adds commute: two runs give the same
//                          bits whatever the arrival order.  Whole 64-pixel groups of one component are carried on by the wave over
//                          its 16 groups before anything is sent.
//
// uaps_rle_count / _encode / _decode: the reference's mask2rle / make_mask exchange format (utilities/utilities.py:36-63), pairs
// (start, length) over the column-major walk of one class's binary plane, 1-based starts.  One lane per (image, column) walks down the
// rows, so that a wave reads 64 consecutive words of a row.  A run starts where the previous pixel of the walk is not of the class and
// ends where the next one is not; the k-th start and the k-th end of a plane belong together, so starts and ends are written
// independently and a last launch turns ends into lengths.
//
// Launches 1 to 3 and the union-find under them live in cc_common.hpp, shared with components.hip; here they run with the policy
// "equal values belong together, the background forms nothing" and without the border flag.
#include <string.h>
#include "cc_common.hpp"
#include "instances_launch.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256;
using namespace uaps::cc;                  // the union-find and the three labelling passes, shared with components.hip

constexpr int kChunk = kThreads;                                                // raster chunk of the numbering scan
constexpr int kMaxGrid = 1 << 24;

using LabelArgs = CcArgs<SameValuePolicy>;

__global__ __launch_bounds__(kThreads) void tile_label_kernel(LabelArgs a) {
    __shared__ long long cls[kTile];
    __shared__ int lab[kTile];
    cc_tile_label(a, cls, lab);
}

__global__ __launch_bounds__(kThreads) void seam_merge_kernel(LabelArgs a) { cc_seam_merge(a); }

__global__ __launch_bounds__(kThreads) void flatten_area_kernel(const int* __restrict__ parent, int* __restrict__ roots, int* area, long HW, long N) {
    cc_flatten_area(parent, roots, area, HW, N, NoMark());
}

struct NumberArgs {
    int B, H, W, chunks, min_area, max_instances;
    const long long* mask;
    const int* roots;       // = labels, still holding the roots
    int* area;              // in: area at the roots; out (number_roots_kernel): the component's number at its root, 0 elsewhere
    int* chunk_off;         // [B][chunks]
    int* count;             // [B]
    long long* table;       // [B][max_instances][9]
};

__device__ __forceinline__ bool survives(const NumberArgs& a, long n, int i) { return a.roots[n] == i && a.area[n] >= a.min_area; }

__global__ __launch_bounds__(kThreads) void chunk_count_kernel(NumberArgs a) {
    __shared__ int red[kWaves];
    const long HW = (long)a.H * a.W;
    const int b = blockIdx.x / a.chunks, ch = blockIdx.x - b * a.chunks;
    const long i = (long)ch * kChunk + threadIdx.x;
    const bool f = i < HW && survives(a, (long)b * HW + i, (int)i);
    const unsigned long long bal = __ballot(f);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) a.chunk_off[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// exclusive prefix of v over the block and the block's total; sm: kWaves ints
__device__ __forceinline__ int block_excl_scan(int v, int* sm, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    __syncthreads();                           // sm is reused by the caller's next round
    if (lane == 63) sm[wave] = incl;
    __syncthreads();
    int off = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) off += w < wave ? sm[w] : 0;
    total = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    return off + incl - v;
}

// block s turns data[s * len .. + len) into its exclusive prefix sums, four words a lane and round, and stores the sum in totals[s]
__global__ __launch_bounds__(kThreads) void scan_segments_kernel(int* data, long len, int* totals) {
    __shared__ int sm[kWaves];
    int* d = data + (long)blockIdx.x * len;
    int carry = 0;
    for (long base = 0; base < len; base += 4 * kThreads) {
        const long i0 = base + 4 * (long)threadIdx.x;
        int v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = i0 + k < len ? d[i0 + k] : 0; s += v[k]; }
        int total;
        int off = carry + block_excl_scan(s, sm, total);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < len) d[i0 + k] = off;
            off += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void number_roots_kernel(NumberArgs a) {
    __shared__ int sm[kWaves];
    const long HW = (long)a.H * a.W;
    const int b = blockIdx.x / a.chunks, ch = blockIdx.x - b * a.chunks;
    const long i = (long)ch * kChunk + threadIdx.x;
    const long n = (long)b * HW + i;
    const bool in = i < HW;
    const bool root = in && a.roots[n] == (int)i;
    const bool f = root && a.area[n] >= a.min_area;
    int total;
    const int k = a.chunk_off[blockIdx.x] + block_excl_scan(f ? 1 : 0, sm, total) + 1;
    if (!root) return;                         // the area word of any other pixel was never raised: it is 0 already
    const int ar = a.area[n];
    a.area[n] = f ? k : 0;
    if (f && k <= a.max_instances) {
        long long* row = a.table + ((long)b * a.max_instances + (k - 1)) * 9;
        row[0] = a.mask[n];
        row[1] = ar;
        row[2] = i / a.W;                      // the first pixel in raster order lies in the component's first row
        row[3] = a.W;                          // x0, y1, x1: neutral elements of final_kernel's atomicMin / atomicMax
        row[4] = 0;
        row[5] = 0;
        row[6] = i;
    }
}

__device__ __forceinline__ long long fixed_q(float v) {
    if (v != v) return 0;
    v = fminf(fmaxf(v, -65536.f), 65536.f);
    return (long long)rintf(v * 16777216.f);
}

struct FinalArgs {
    int B, H, W, max_instances;
    int* labels;            // in: roots; out: numbers
    const int* number;      // the area scratch after number_roots_kernel
    const float* map0;
    const float* map1;
    long long* table;
};

struct RowAcc { int x0, x1, y1; long long q0, q1; };
__device__ __forceinline__ void flush_row(const FinalArgs& a, long b, int kk, const RowAcc& r) {
    unsigned long long* row = reinterpret_cast<unsigned long long*>(a.table + (b * a.max_instances + (kk - 1)) * 9);
    atomicMin(row + 3, (unsigned long long)r.x0);
    atomicMax(row + 4, (unsigned long long)r.y1);
    atomicMax(row + 5, (unsigned long long)r.x1);
    if (a.map0) atomicAdd(row + 7, (unsigned long long)r.q0);
    if (a.map1) atomicAdd(row + 8, (unsigned long long)r.q1);
}

__global__ __launch_bounds__(kThreads) void final_kernel(FinalArgs a) {
    const long HW = (long)a.H * a.W, N = (long)a.B * HW;
    const int lane = threadIdx.x & 63;
    const long w0 = ((long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * (kSpan * 64);
    long pend_b = -1;                          // pending: whole groups of one component, carried by the wave (uniform); lane 0 flushes
    int pend_k = 0;
    RowAcc pend = {0, 0, 0, 0, 0};
    for (int it = 0; it < kSpan; ++it) {
        const long base = w0 + (long)it * 64;
        if (base >= N) break;                  // (wave-uniform)
        const long n = base + lane;
        int kk = -1, y = 0, x = 0;
        long b = 0;
        long long q0 = 0, q1 = 0;
        if (n < N) {
            b = n / HW;
            const long i = n - b * HW;
            y = (int)(i / a.W); x = (int)(i - (long)y * a.W);
            const int r = a.labels[n];
            const int k = r >= 0 ? a.number[b * HW + r] : 0;
            a.labels[n] = k;
            kk = k <= a.max_instances ? k : 0;          // components numbered above max_instances keep their labels and get no row
            if (kk > 0) {
                if (a.map0) q0 = fixed_q(a.map0[n]);
                if (a.map1) q1 = fixed_q(a.map1[n]);
            }
        }
        const int prev = __shfl_up(kk, 1, 64);
        const bool head = lane == 0 || prev != kk || x == 0;
        const unsigned long long heads = __ballot(head);
        const int end = run_end(heads, lane);
        // sum over [lane, end]: after the step of width o a lane holds the sum of min(2 o, end - lane + 1) lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long t0 = __shfl_down(q0, o, 64), t1 = __shfl_down(q1, o, 64);
            if (lane + o <= end) { q0 += t0; q1 += t1; }
        }
        const RowAcc mine = {x, x + (end - lane) + 1, y + 1, q0, q1};
        const int k0 = __shfl(kk, 0, 64);
        const long b0 = __shfl(b, 0, 64);
        if (heads == 1ull && k0 > 0) {         // the whole group is one run of one component (so all 64 lanes are valid, in one row)
            if (pend_k == k0 && pend_b == b0) {
                pend.x0 = min(pend.x0, mine.x0); pend.x1 = max(pend.x1, mine.x1); pend.y1 = max(pend.y1, mine.y1);
                pend.q0 += mine.q0; pend.q1 += mine.q1;
            } else {
                if (pend_k > 0 && lane == 0) flush_row(a, pend_b, pend_k, pend);
                pend_b = b0; pend_k = k0; pend = mine;
            }
            continue;
        }
        if (pend_k > 0 && lane == 0) flush_row(a, pend_b, pend_k, pend);
        pend_k = 0;
        if (head && kk > 0) flush_row(a, b, kk, mine);
    }
    if (pend_k > 0 && lane == 0) flush_row(a, pend_b, pend_k, pend);
}

inline long chunks_of(long HW) { return (HW + kChunk - 1) / kChunk; }
inline int grid_of(long items) { return grid_for(items, kMaxGrid); }

// the dimension rules of uaps_label_instances: 0 or the code
inline int check_dims(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if ((double)H * W >= kTooBig || (double)B * H * W * 8.0 >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}
inline size_t workspace_for(int B, int H, int W) {
    const size_t N = (size_t)B * H * W;
    return 2 * align256(4 * N) + align256(4 * (size_t)B * chunks_of((long)H * W));
}

// ---------------------------------------------------------------------------------------------- run-length masks
constexpr int kRleMax = UAPS_RLE_MAX_CLASSES;

struct RleArgs {
    int B, H, W, nc;
    long long cls[kRleMax];
    const long long* mask;
    int* col_off;           // [B][nc][W] (+ 1: the total)
    int* pairs;
};

// WRITE == false: the number of runs of class c that START in column x of image b -> col_off[(b nc + c) W + x].
// WRITE == true:  col_off holds the exclusive prefix sums of those; starts go to pairs[2 k], exclusive 1-based ends to pairs[2 k + 1].
//                 The ends of a column begin one run earlier than its starts where a run runs on across the column's upper edge.
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void rle_walk_kernel(RleArgs a) {
    const long cols = (long)a.B * a.W, HW = (long)a.H * a.W;
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < cols; g += (long)gridDim.x * kThreads) {
        const int b = (int)(g / a.W), x = (int)(g - (long)b * a.W);
        const long long* m = a.mask + (long)b * HW + x;
        const bool has_prev = x > 0, has_next = x < a.W - 1;
        const long long before = has_prev ? m[(long)(a.H - 1) * a.W - 1] : 0;       // (H-1, x-1)
        const long long after = has_next ? m[1] : 0;                                // (0, x+1)
        int ks[kRleMax], ke[kRleMax];
        for (int c = 0; c < a.nc; ++c) {
            ks[c] = 0; ke[c] = 0;
            if (WRITE) {
                ks[c] = a.col_off[((long)b * a.nc + c) * a.W + x];
                ke[c] = ks[c] - ((has_prev && before == a.cls[c] && m[0] == a.cls[c]) ? 1 : 0);
            }
        }
        long long prev = before, cur = m[0];
        bool prev_ok = has_prev;
        for (int y = 0; y < a.H; ++y) {
            const bool next_ok = y < a.H - 1 || has_next;
            const long long next = y < a.H - 1 ? m[(long)(y + 1) * a.W] : after;
            const int pos = x * a.H + y + 1;                                        // 1-based, column-major
            for (int c = 0; c < a.nc; ++c) {
                if (cur != a.cls[c]) continue;
                if (!(prev_ok && prev == cur)) {
                    if (WRITE) a.pairs[2 * (long)ks[c]] = pos;
                    ++ks[c];
                }
                if (WRITE && !(next_ok && next == cur)) {
                    a.pairs[2 * (long)ke[c] + 1] = pos + 1;
                    ++ke[c];
                }
            }
            prev = cur; prev_ok = true; cur = next;
        }
        if (!WRITE)
            for (int c = 0; c < a.nc; ++c) a.col_off[((long)b * a.nc + c) * a.W + x] = ks[c];
    }
}

__global__ __launch_bounds__(kThreads) void rle_lengths_kernel(int* pairs, const int* total) {
    const long runs = *total;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < runs; k += (long)gridDim.x * kThreads) pairs[2 * k + 1] -= pairs[2 * k];
}

struct DecodeArgs {
    int B, H, W, nc, c;
    long long value;
    long runs;
    const int* pairs;
    const int* offsets;     // [B nc + 1]
    void* out;
};

// one wave per run; only the runs of class index a.c (one launch per class, in order: later classes win)
template <typename T>
__global__ __launch_bounds__(kThreads) void rle_decode_kernel(DecodeArgs a) {
    const int lane = threadIdx.x & 63;
    const long HW = (long)a.H * a.W, segs = (long)a.B * a.nc;
    const long waves = (long)gridDim.x * kWaves;
    for (long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); r < a.runs; r += waves) {
        long lo = 0, hi = segs;                 // the last segment whose offset is <= r (empty segments share an offset)
        while (hi - lo > 1) {
            const long mid = (lo + hi) / 2;
            if (a.offsets[mid] <= r) lo = mid; else hi = mid;
        }
        if ((int)(lo % a.nc) != a.c) continue;
        const long b = lo / a.nc;
        const long start = (long)a.pairs[2 * r] - 1, len = a.pairs[2 * r + 1];
        T* out = static_cast<T*>(a.out) + b * HW;
        for (long p = start + lane; p < start + len; p += 64) {
            if (p < 0 || p >= HW) continue;     // (the host refuses such runs where it sees them; never write outside the plane)
            out[(p % a.H) * a.W + p / a.H] = (T)a.value;
        }
    }
}

// the checks the three entry points share; 0 or the code.  `c` receives the caller's struct, size-versioned.
inline int read_rle(const uaps_rle_call* call, uaps_rle_call& c) {
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0) return UAPS_EINVAL;
    if (c.n_classes < 1 || c.n_classes > kRleMax) return UAPS_ERANGE;
    if ((double)c.H * c.W >= kTooBig || (double)c.B * c.H * c.W * 8.0 >= kTooBig) return UAPS_ERANGE;
    if ((double)c.B * c.n_classes * c.W * 4.0 >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}
inline RleArgs rle_args(const uaps_rle_call& c) {
    RleArgs a;
    memset(&a, 0, sizeof a);
    a.B = c.B; a.H = c.H; a.W = c.W; a.nc = c.n_classes;
    for (int k = 0; k < c.n_classes; ++k) a.cls[k] = c.classes[k];
    a.mask = (const long long*)c.mask; a.col_off = c.col_offsets; a.pairs = c.pairs;
    return a;
}
}  // namespace

extern "C" int uaps_instances_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    const int rc = check_dims(B, H, W);
    if (rc) return rc;
    *bytes = workspace_for(B, H, W);
    return UAPS_OK;
}

extern "C" int uaps_label_instances(const uaps_instances_call* call) {
    uaps_instances_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.mask || !c.labels || !c.count || !c.table || !c.workspace) return UAPS_EINVAL;
    if (c.map1 && !c.map0) return UAPS_EINVAL;
    if ((c.connectivity != 4 && c.connectivity != 8) || c.min_area < 1 || c.max_instances < 1) return UAPS_EINVAL;
    if (c.has_background != 0 && c.has_background != 1) return UAPS_EINVAL;
    const int rc = check_dims(c.B, c.H, c.W);
    if (rc) return rc;
    if ((double)c.B * c.max_instances * 72.0 >= kTooBig) return UAPS_ERANGE;
    if (c.workspace_bytes < workspace_for(c.B, c.H, c.W)) return UAPS_EWORKSPACE;
    return uaps::label_launches(c);
}

// The launches of uaps_label_instances on a call whose every check has passed (instances_launch.hpp): split.hip runs them on its own
// code map, with a part of its workspace as theirs.
size_t uaps::label_workspace_bytes(int B, int H, int W) { return workspace_for(B, H, W); }

int uaps::label_launches(const uaps_instances_call& c) {
    const long HW = (long)c.H * c.W, N = (long)c.B * HW;
    const int chunks = (int)chunks_of(HW);
    char* ws = static_cast<char*>(c.workspace);
    int* parent = reinterpret_cast<int*>(ws);
    int* area = reinterpret_cast<int*>(ws + align256(4 * (size_t)N));
    int* chunk_off = reinterpret_cast<int*>(ws + 2 * align256(4 * (size_t)N));
    hipStream_t st = (hipStream_t)c.stream;
    uaps::account_bytes((double)N * (8.0 + 4.0 + (c.map0 ? 4.0 : 0.0) + (c.map1 ? 4.0 : 0.0)) + (double)c.B * (4.0 + 72.0 * c.max_instances));

    const hipError_t e = hipMemsetAsync(c.table, 0, (size_t)c.B * c.max_instances * 72, st);
    if (e != hipSuccess) return (int)e;
    LabelArgs la;
    la.Q = c.B; la.H = c.H; la.W = c.W; la.ntx = (c.W + kTW - 1) / kTW; la.nty = (c.H + kTH - 1) / kTH;
    la.conn8 = c.connectivity == 8; la.pol.has_bg = c.has_background; la.pol.bg = c.background;
    la.mask = (const long long*)c.mask; la.parent = parent; la.area = area;
    const long tiles = (long)c.B * la.ntx * la.nty;             // < 2^28: every tile holds a pixel
    UAPS_LAUNCH_MAIN(tile_label_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, la);
    const long seam = (long)c.B * ((long)(la.nty - 1) * c.W + (long)(la.ntx - 1) * c.H);
    if (seam > 0) hipLaunchKernelGGL(seam_merge_kernel, dim3(grid_of(seam)), dim3(kThreads), 0, st, la);
    hipLaunchKernelGGL(flatten_area_kernel, dim3(span_grid(N)), dim3(kThreads), 0, st, (const int*)parent, c.labels, area, HW, N);
    NumberArgs na;
    na.B = c.B; na.H = c.H; na.W = c.W; na.chunks = chunks; na.min_area = c.min_area; na.max_instances = c.max_instances;
    na.mask = (const long long*)c.mask; na.roots = c.labels; na.area = area; na.chunk_off = chunk_off; na.count = c.count;
    na.table = (long long*)c.table;
    const unsigned nblk = (unsigned)((long)c.B * chunks);       // <= N / 256 + B
    hipLaunchKernelGGL(chunk_count_kernel, dim3(nblk), dim3(kThreads), 0, st, na);
    hipLaunchKernelGGL(scan_segments_kernel, dim3(c.B), dim3(kThreads), 0, st, chunk_off, (long)chunks, c.count);
    hipLaunchKernelGGL(number_roots_kernel, dim3(nblk), dim3(kThreads), 0, st, na);
    FinalArgs fa;
    fa.B = c.B; fa.H = c.H; fa.W = c.W; fa.max_instances = c.max_instances;
    fa.labels = c.labels; fa.number = area; fa.map0 = c.map0; fa.map1 = c.map1; fa.table = (long long*)c.table;
    hipLaunchKernelGGL(final_kernel, dim3(span_grid(N)), dim3(kThreads), 0, st, fa);
    return (int)hipGetLastError();
}

extern "C" int uaps_rle_count(const uaps_rle_call* call) {
    uaps_rle_call c;
    const int rc = read_rle(call, c);
    if (rc) return rc;
    if (!c.mask || !c.col_offsets) return UAPS_EINVAL;
    const RleArgs a = rle_args(c);
    hipStream_t st = (hipStream_t)c.stream;
    const long n = (long)c.B * c.n_classes * c.W;
    uaps::account_bytes(8.0 * c.B * c.H * c.W + 4.0 * (double)n);
    UAPS_LAUNCH_MAIN(rle_walk_kernel<false>, dim3(grid_of((long)c.B * c.W)), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(scan_segments_kernel, dim3(1), dim3(kThreads), 0, st, c.col_offsets, n, c.col_offsets + n);
    return (int)hipGetLastError();
}

extern "C" int uaps_rle_encode(const uaps_rle_call* call) {
    uaps_rle_call c;
    const int rc = read_rle(call, c);
    if (rc) return rc;
    if (!c.mask || !c.col_offsets || !c.pairs) return UAPS_EINVAL;
    const RleArgs a = rle_args(c);
    hipStream_t st = (hipStream_t)c.stream;
    const long n = (long)c.B * c.n_classes * c.W;
    uaps::account_bytes(8.0 * c.B * c.H * c.W + 4.0 * (double)n);
    UAPS_LAUNCH_MAIN(rle_walk_kernel<true>, dim3(grid_of((long)c.B * c.W)), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(rle_lengths_kernel, dim3(grid_of((long)c.B * c.H * c.W / 64)), dim3(kThreads), 0, st, c.pairs, (const int*)(c.col_offsets + n));
    return (int)hipGetLastError();
}

extern "C" int uaps_rle_decode(const uaps_rle_call* call) {
    uaps_rle_call c;
    const int rc = read_rle(call, c);
    if (rc) return rc;
    if (!c.out || !c.offsets || c.n_runs < 0 || (c.n_runs > 0 && !c.pairs)) return UAPS_EINVAL;
    if (c.out_uint8 != 0 && c.out_uint8 != 1) return UAPS_EINVAL;
    if ((double)c.n_runs * 8.0 >= kTooBig) return UAPS_ERANGE;
    if (c.out_uint8)
        for (int k = 0; k < c.n_classes; ++k)
            if (c.classes[k] < 0 || c.classes[k] > 255) return UAPS_ERANGE;
    hipStream_t st = (hipStream_t)c.stream;
    const size_t N = (size_t)c.B * c.H * c.W;
    uaps::account_bytes(8.0 * (double)c.n_runs + (c.out_uint8 ? 1.0 : 8.0) * (double)N);
    const hipError_t e = hipMemsetAsync(c.out, 0, N * (c.out_uint8 ? 1 : 8), st);
    if (e != hipSuccess) return (int)e;
    if (c.n_runs == 0) return UAPS_OK;
    DecodeArgs a;
    a.B = c.B; a.H = c.H; a.W = c.W; a.nc = c.n_classes; a.runs = (long)c.n_runs; a.pairs = c.pairs; a.offsets = c.offsets; a.out = c.out;
    const int grid = grid_for(((long)c.n_runs + kWaves - 1) / kWaves * kThreads, kMaxGrid);
    for (int k = 0; k < c.n_classes; ++k) {
        a.c = k; a.value = c.classes[k];
        if (c.out_uint8) hipLaunchKernelGGL(rle_decode_kernel<uint8_t>, dim3(grid), dim3(kThreads), 0, st, a);
        else hipLaunchKernelGGL(rle_decode_kernel<long long>, dim3(grid), dim3(kThreads), 0, st, a);
    }
    return (int)hipGetLastError();
}
