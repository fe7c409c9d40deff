// Boundary metrics for gfx950 (include/uaps_hip.h, uaps_edt_sq / uaps_surface_distances): an exact squared Euclidean distance
// transform and the directed surface distances of two label maps, reduced on the device to one int64 row per (image, class).
//
// The transform is the separable one: D2(y, x) = min over x' of ((x - x')^2 + g(y, x')^2), g = the distance along the column to the
// nearest feature pixel.  Everything is an integer; squared distances reach 2 * 4095^2 > 2^24, so no fp32 touches one.
//   column sweep   a lane owns one row segment of one column (of one side): down, then up, the carries between the segments of a
//                  column through LDS (col_kernel).  One lane per whole column is a chain of H dependent memory round trips with
//                  B * W lanes on the whole chip (measured: 377 us of a 500 us call at 16 x 256 x 256).  Rows are taken kRows at
//                  a time so that a batch's loads are in flight together.  g is uint16, 65535 = none in this column.  Surface
//                  membership is decided from the label and its four neighbours on the fly; on the way up "g == 0" says it.
//   row pass       a workgroup stages the squares of one row of g in LDS (none -> 2^30: 2^30 + 4095^2 < 2^31).  A lane scans
//                  outwards from its pixel and stops once dx^2 reaches its best value.
//   surface        only lanes on a surface pixel of one side scan, over the other side's row; count, maximum, sum of
//                  floor(2^16 sqrt(d2)) and the within-tolerance count go through a wave and workgroup reduction into 64-bit integer
//                  atomics (add and max: the result does not depend on order).  d2, or -1 where there is no surface pixel, is left
//                  in the workspace for the selection.
//   selection      squared distances are below 2^25: three histogram passes over 9 + 8 + 8 bits, for the two ranks at once.  A
//                  workgroup histograms kChunk values in LDS (a wave whose lanes all hit one bin sends one add) and flushes the
//                  bins it touched with integer atomics; one workgroup per pair then finds each rank's bin with a block scan.
// No launch waits for another workgroup; launch boundaries are the only coherence points.
#include "call_common.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::align256;

constexpr int kExtent = UAPS_SURFACE_MAX_EXTENT;
constexpr int kCols = UAPS_SURFACE_COLUMNS;
constexpr int kNone = 65535;                    // g: no feature in this column
constexpr int kInf = UAPS_EDT_NO_FEATURE;       // its "square": above every real squared distance, and kInf + 4095^2 < 2^31
constexpr int kMaxSeg = 16, kColMaxThreads = kMaxSeg * 64;   // a column is swept in up to 16 row segments, one wave each
constexpr int kRows = 4;                        // rows of a column in flight together
constexpr int kBins = 512, kPasses = 3;
constexpr int kChunk = kThreads * 16;           // values per workgroup of a histogram pass
constexpr int kOutside = -2;                    // a neighbour outside the image: equal to no label

// a label as an int: [0, UAPS_MAX_CLASSES) or -1 (belongs to no class)
__device__ __forceinline__ int load_label(const void* __restrict__ p, long i, int esz) {
    long long v;
    if (esz == 1) v = static_cast<const uint8_t*>(p)[i];
    else if (esz == 4) v = static_cast<const int*>(p)[i];
    else v = static_cast<const long long*>(p)[i];
    return (v >= 0 && v < UAPS_MAX_CLASSES) ? (int)v : -1;
}
__device__ __forceinline__ bool load_nonzero(const void* __restrict__ p, long i, int esz) {
    if (esz == 1) return static_cast<const uint8_t*>(p)[i] != 0;
    if (esz == 4) return static_cast<const int*>(p)[i] != 0;
    return static_cast<const long long*>(p)[i] != 0;
}
__device__ __forceinline__ int step(int cnt, bool feature) { return feature ? 0 : (cnt == kNone ? kNone : cnt + 1); }

struct ColArgs {
    int B, H, W, nseg;      // nseg: row segments per column = waves per workgroup
    int esz0, esz1;
    const void* lab0;       // prediction (surface) / mask (transform)
    const void* lab1;       // target
    uint16_t* g;            // [B][C][2][H][W] (surface) / [B][H][W] (transform)
};

// Workgroup = (image, side, strip of 64 columns); wave = one of nseg row segments of the strip; lane = one column of it.
//   A  down the segment: the feature flags of every class from the labels, the distance to the nearest feature above INSIDE the
//      segment -> g; the count at the segment's last row -> tail (LDS).
//   B  up the segment over g: what A left none takes the carry from the segments above (tail + the rows between); the distance to
//      the nearest feature below inside the segment is formed on the way ("g == 0" says feature); g := the smaller of the two; the
//      count at the segment's first row -> head (LDS).
//   C  the rows behind the segment's last feature, the only ones whose nearest feature below lies in a later segment, take the
//      carry from below (head + the rows between).
// A lane reads back only what it wrote itself; the two barriers order the LDS words.  EDT: one plane, the feature is a zero pixel.
template <int C, bool EDT>
__global__ __launch_bounds__(kColMaxThreads) void col_kernel(ColArgs a) {
    __shared__ uint16_t tail[kMaxSeg][C][64], head[kMaxSeg][C][64];
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int strips = (a.W + 63) / 64;
    const int strip = (int)(blockIdx.x % strips);
    const long t = blockIdx.x / strips;
    const int s = EDT ? 0 : (int)(t & 1);
    const long b = EDT ? t : t >> 1;
    const int x = strip * 64 + lane;
    const int S = (a.H + a.nseg - 1) / a.nseg;
    const int y_lo = min(seg * S, a.H), y_hi = min(y_lo + S, a.H);
    const bool active = x < a.W && y_lo < y_hi;
    const long HW = (long)a.H * a.W, stride = EDT ? 0 : 2 * HW;
    const void* __restrict__ lab = s ? a.lab1 : a.lab0;
    const int esz = s ? a.esz1 : a.esz0;
    const long base = b * HW + x;
    uint16_t* __restrict__ g = a.g + (EDT ? b * HW : (b * C * 2 + s) * HW) + x;
    int cnt[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cnt[c] = kNone;
    if (active) {
        const bool has_l = x > 0, has_r = x < a.W - 1;
        int up = (!EDT && y_lo > 0) ? load_label(lab, base + (long)(y_lo - 1) * a.W, esz) : kOutside;
        for (int y0 = y_lo; y0 < y_hi; y0 += kRows) {
            int mid[kRows + 1], lf[kRows], rt[kRows];
#pragma unroll
            for (int r = 0; r <= kRows; ++r) {
                const bool in = y0 + r < a.H && (!EDT || r < kRows);
                if (EDT) mid[r] = in && load_nonzero(lab, base + (long)(y0 + r) * a.W, esz) ? 1 : 0;
                else mid[r] = in ? load_label(lab, base + (long)(y0 + r) * a.W, esz) : kOutside;
            }
            if (!EDT) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) {
                    const bool in = y0 + r < y_hi;
                    lf[r] = in && has_l ? load_label(lab, base + (long)(y0 + r) * a.W - 1, esz) : kOutside;
                    rt[r] = in && has_r ? load_label(lab, base + (long)(y0 + r) * a.W + 1, esz) : kOutside;
                }
            }
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                if (y0 + r >= y_hi) break;
                const int cur = mid[r];
                const bool open = EDT ? cur == 0 : (up != cur || mid[r + 1] != cur || lf[r] != cur || rt[r] != cur);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    cnt[c] = step(cnt[c], open && (EDT || cur == c));
                    g[c * stride + (long)(y0 + r) * a.W] = (uint16_t)cnt[c];
                }
                up = cur;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) tail[seg][c][lane] = (uint16_t)cnt[c];
    __syncthreads();
    int upc[C];
    if (active) {
        int carry[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            carry[c] = kNone;
            upc[c] = kNone;
            for (int sp = seg - 1; sp >= 0; --sp) {
                const int tv = tail[sp][c][lane];
                if (tv != kNone) { carry[c] = tv + (y_lo - min((sp + 1) * S, a.H)); break; }
            }
        }
        for (int y0 = y_hi - 1; y0 >= y_lo; y0 -= kRows) {
            int gd[kRows][C];
#pragma unroll
            for (int r = 0; r < kRows; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c) gd[r][c] = y0 - r >= y_lo ? g[c * stride + (long)(y0 - r) * a.W] : 0;
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const int y = y0 - r;
                if (y < y_lo) break;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    upc[c] = step(upc[c], gd[r][c] == 0);
                    const int down = gd[r][c] != kNone ? gd[r][c] : (carry[c] == kNone ? kNone : carry[c] + (y - y_lo + 1));
                    const int out = min(down, upc[c]);
                    if (out != gd[r][c]) g[c * stride + (long)y * a.W] = (uint16_t)out;
                }
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) upc[c] = kNone;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) head[seg][c][lane] = (uint16_t)upc[c];
    __syncthreads();
    if (!active) return;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int below = kNone;
        for (int sp = seg + 1; sp < a.nseg; ++sp) {
            const int hv = head[sp][c][lane];
            if (hv != kNone) { below = hv + (min(sp * S, a.H) - y_hi); break; }
        }
        if (below == kNone) continue;
        const int n = cnt[c] == kNone ? y_hi - y_lo : cnt[c];      // the rows behind the segment's last feature
        for (int y0 = y_hi - 1; y0 >= y_hi - n; y0 -= kRows) {
            int gv[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) gv[r] = y0 - r >= y_hi - n ? g[c * stride + (long)(y0 - r) * a.W] : 0;
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const int y = y0 - r, cand = below + (y_hi - y);
                if (y >= y_hi - n && cand < gv[r]) g[c * stride + (long)y * a.W] = (uint16_t)cand;
            }
        }
    }
}

inline int segments_for(int H) { const int n = (H + 15) / 16; return n < 1 ? 1 : (n > kMaxSeg ? kMaxSeg : n); }

__device__ __forceinline__ int square_of(int g) { return g == kNone ? kInf : g * g; }

// min over x' of (x - x')^2 + sq[x'], outwards from x, until dx^2 alone reaches the best value
__device__ __forceinline__ int scan_min(const int* sq, int x, int W) {
    int best = sq[x];
    const int reach = max(x, W - 1 - x);
    for (int d = 1; d <= reach; ++d) {
        const int dd = d * d;
        if (dd >= best) break;
        if (x - d >= 0) best = min(best, sq[x - d] + dd);
        if (x + d < W) best = min(best, sq[x + d] + dd);
    }
    return best;
}

__global__ __launch_bounds__(kThreads) void edt_row_kernel(const uint16_t* __restrict__ g, int* __restrict__ out, int W) {
    extern __shared__ int sq[];
    const long row = (long)blockIdx.x * W;
    for (int x = threadIdx.x; x < W; x += kThreads) sq[x] = square_of(g[row + x]);
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += kThreads) out[row + x] = scan_min(sq, x, W);
}

// floor(2^16 sqrt(d2)) = the integer square root of d2 << 32: a double-precision start, corrected by integer comparison
__device__ __forceinline__ long long isqrt16(int d2) {
    const unsigned long long v = (unsigned long long)(unsigned)d2 << 32;
    unsigned long long r = (unsigned long long)(sqrt((double)d2) * 65536.0);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return (long long)r;
}

struct RowArgs {
    int H, W, has_tol;
    long long tol;
    const uint16_t* g;          // [B][C][2][H][W]
    int* d2;                    // [B][C][2][H][W]: the directed squared distance at surface pixels, -1 elsewhere
    unsigned long long* table;  // [B][C][kCols], zeroed
};

// workgroup = one row of one (image, class); values 0/1: counts, 2/3: maxima, 4/5: sum16, 6/7: within
__global__ __launch_bounds__(kThreads) void surface_row_kernel(RowArgs a) {
    extern __shared__ int sq[];                 // [2][W]
    __shared__ long long red[kWaves][8];
    const long bc = blockIdx.x / a.H;
    const int y = (int)(blockIdx.x - bc * a.H);
    const long HW = (long)a.H * a.W, off = bc * 2 * HW + (long)y * a.W;
    const uint16_t* __restrict__ g0 = a.g + off;
    int* __restrict__ d0 = a.d2 + off;
    for (int x = threadIdx.x; x < a.W; x += kThreads) {
        sq[x] = square_of(g0[x]);
        sq[a.W + x] = square_of(g0[HW + x]);
    }
    __syncthreads();
    long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int x = threadIdx.x; x < a.W; x += kThreads) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int out = -1;
            if (sq[s * a.W + x] == 0) {
                out = scan_min(sq + (1 - s) * a.W, x, a.W);
                v[s] += 1;
                v[2 + s] = max(v[2 + s], (long long)out);
                v[4 + s] += isqrt16(out);
                v[6 + s] += (a.has_tol && (long long)out <= a.tol) ? 1 : 0;
            }
            d0[s * HW + x] = out;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long t = __shfl_xor(v[k], o, 64);
            v[k] = (k == 2 || k == 3) ? max(v[k], t) : v[k] + t;
        }
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 8; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    const int k = threadIdx.x;
    if (k < 8) {
        const bool is_max = k == 2 || k == 3;
        long long r = red[0][k];
        for (int w = 1; w < kWaves; ++w) r = is_max ? max(r, red[w][k]) : r + red[w][k];
        if (r > 0) {
            unsigned long long* dst = a.table + bc * kCols + k;
            if (is_max) atomicMax(dst, (unsigned long long)r);
            else atomicAdd(dst, (unsigned long long)r);
        }
    }
}

struct SelState {
    unsigned long long rank[2];     // the rank still to find among the values that share prefix[k]
    unsigned prefix[2];             // the bits of the two order statistics found so far
    int valid, pad;
};

// one lane per (image, class): the ranks from N; a pair without a surface on either side keeps its counts alone
__global__ __launch_bounds__(kThreads) void surface_ranks_kernel(long long* __restrict__ table, SelState* __restrict__ st, int BC, double frac) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= BC) return;
    long long* row = table + (long)i * kCols;
    SelState s;
    s.prefix[0] = s.prefix[1] = 0;
    s.rank[0] = s.rank[1] = 0;
    s.pad = 0;
    s.valid = row[0] > 0 && row[1] > 0;
    if (!s.valid) {
        for (int k = 2; k < kCols; ++k) row[k] = 0;
    } else {
        const long long N = row[0] + row[1];
        const double h = (double)(N - 1) * frac;
        long long lo = (long long)floor(h);
        lo = lo < 0 ? 0 : (lo > N - 1 ? N - 1 : lo);
        const long long hi = lo + 1 < N - 1 ? lo + 1 : N - 1;
        row[8] = lo;
        row[9] = hi;
        s.rank[0] = (unsigned long long)lo;
        s.rank[1] = (unsigned long long)hi;
    }
    st[i] = s;
}

__host__ __device__ constexpr int pass_shift(int p) { return p == 0 ? 16 : (p == 1 ? 8 : 0); }
__host__ __device__ constexpr int pass_bits(int p) { return p == 0 ? 9 : 8; }

// one LDS add per lane, or one per wave where every counted lane of the wave hits the same bin (masks that nearly agree: all of them)
__device__ __forceinline__ void wave_hist_add(unsigned* h, bool ok, int digit, int lane) {
    const unsigned long long act = __ballot(ok);
    if (!act) return;
    const int first = __builtin_ctzll(act);
    const int d0 = __shfl(digit, first, 64);
    if (__ballot(ok && digit != d0) == 0ull) {
        if (lane == first) atomicAdd(h + d0, (unsigned)__popcll(act));
    } else if (ok) {
        atomicAdd(h + digit, 1u);
    }
}

struct SelArgs {
    long HW;
    int chunks;                 // workgroups per pair in a histogram pass
    const int* d2;              // [BC][2][HW]
    const SelState* st;
    unsigned* hist;             // [BC][kPasses][2][kBins], zeroed
};

template <int P>
__global__ __launch_bounds__(kThreads) void surface_hist_kernel(SelArgs a) {
    __shared__ unsigned h[2][kBins];
    const long bc = blockIdx.x / a.chunks;
    const int chunk = (int)(blockIdx.x - bc * a.chunks);
    const SelState st = a.st[bc];
    if (!st.valid) return;                      // (uniform over the workgroup)
    const bool two = st.prefix[1] != st.prefix[0];
    for (int j = threadIdx.x; j < 2 * kBins; j += kThreads) (&h[0][0])[j] = 0;
    __syncthreads();
    constexpr int shift = pass_shift(P), bits = pass_bits(P);
    const long n = 2 * a.HW;
    const int* __restrict__ v = a.d2 + bc * n;
    const long i0 = (long)chunk * kChunk;
    const int lane = threadIdx.x & 63;
#pragma unroll 4
    for (int it = 0; it < kChunk / kThreads; ++it) {
        const long i = i0 + (long)it * kThreads + threadIdx.x;
        const int val = i < n ? v[i] : -1;
        const unsigned top = (unsigned)val >> (shift + bits);   // (-1 is excluded by `val >= 0`)
        const int digit = (int)(((unsigned)val >> shift) & ((1u << bits) - 1u));
        wave_hist_add(h[0], val >= 0 && top == st.prefix[0], digit, lane);
        if (two) wave_hist_add(h[1], val >= 0 && top == st.prefix[1], digit, lane);
    }
    __syncthreads();
    unsigned* out = a.hist + (bc * kPasses + P) * 2 * kBins;
    for (int j = threadIdx.x; j < (two ? 2 : 1) * kBins; j += kThreads) {
        const unsigned c = (&h[0][0])[j];
        if (c) atomicAdd(out + j, c);
    }
}

// exclusive prefix of v over the block; sm: kWaves words
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    __syncthreads();                            // sm is reused by the next scan
    if (lane == 63) sm[wave] = incl;
    __syncthreads();
    unsigned off = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) off += w < wave ? sm[w] : 0u;
    return off + incl - v;
}

// workgroup = one pair: the bin of pass P that holds each rank; the last pass writes q_lo and q_hi
template <int P>
__global__ __launch_bounds__(kThreads) void surface_pick_kernel(SelState* __restrict__ states, const unsigned* __restrict__ hist, long long* __restrict__ table) {
    __shared__ unsigned sm[kWaves];
    __shared__ unsigned digit_of[2];
    __shared__ unsigned long long rank_of[2];
    const long bc = blockIdx.x;
    const SelState st = states[bc];
    if (!st.valid) return;
    const int t = threadIdx.x;
    for (int k = 0; k < 2; ++k) {
        const unsigned* h = hist + ((bc * kPasses + P) * 2 + ((k == 1 && st.prefix[1] != st.prefix[0]) ? 1 : 0)) * kBins;
        const unsigned c0 = h[2 * t], c1 = h[2 * t + 1];
        const unsigned long long excl = block_excl_scan(c0 + c1, sm);
        const unsigned long long r = st.rank[k];
        if (r >= excl && r < excl + c0) { digit_of[k] = 2 * t; rank_of[k] = r - excl; }
        else if (r >= excl + c0 && r < excl + c0 + c1) { digit_of[k] = 2 * t + 1; rank_of[k] = r - excl - c0; }
    }
    __syncthreads();
    if (t == 0) {
        SelState s = st;
        for (int k = 0; k < 2; ++k) {
            s.prefix[k] = (st.prefix[k] << pass_bits(P)) | digit_of[k];
            s.rank[k] = rank_of[k];
            if (P == kPasses - 1) table[bc * kCols + 10 + k] = s.prefix[k];
        }
        states[bc] = s;
    }
}

// scores [B][C][H][W] -> uint8 labels: the lowest index among equal scores (strict >)
__global__ __launch_bounds__(kThreads) void argmax_kernel(const float* __restrict__ z, uint8_t* __restrict__ out, int C, long HW, long N) {
    for (long n = (long)blockIdx.x * kThreads + threadIdx.x; n < N; n += (long)gridDim.x * kThreads) {
        const long b = n / HW, i = n - b * HW;
        const float* p = z + b * C * HW + i;
        float best = p[0];
        int idx = 0;
        for (int c = 1; c < C; ++c) {
            const float q = p[(long)c * HW];
            if (q > best) { best = q; idx = c; }
        }
        out[n] = (uint8_t)idx;
    }
}

inline bool dtype_ok(int d) { return d == UAPS_LABEL_U8 || d == UAPS_LABEL_I32 || d == UAPS_LABEL_I64; }

inline int check_extent(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if (H > kExtent || W > kExtent) return UAPS_ERANGE;
    return UAPS_OK;
}

inline int check_edt(int B, int H, int W) {
    const int rc = check_extent(B, H, W);
    if (rc) return rc;
    if ((double)B * H * W * 8.0 >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}

// surface: g, d2, histograms, states, the arg-max labels
struct SurfaceLayout { size_t g, d2, hist, st, lab, total; };
inline SurfaceLayout surface_layout(int B, int C, int H, int W) {
    const size_t n = (size_t)B * C * 2 * H * W, bc = (size_t)B * C;
    SurfaceLayout l;
    l.g = 0;
    l.d2 = l.g + align256(2 * n);
    l.hist = l.d2 + align256(4 * n);
    l.st = l.hist + align256(4 * bc * kPasses * 2 * kBins);
    l.lab = l.st + align256(sizeof(SelState) * bc);
    l.total = l.lab + align256((size_t)B * H * W);
    return l;
}
inline int check_surface(int B, int C, int H, int W) {
    const int rc = check_extent(B, H, W);
    if (rc) return rc;
    if (C < 1 || C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
    const double px = (double)B * H * W, bc = (double)B * C;
    if (px * 8.0 >= kTooBig || px * C * 4.0 >= kTooBig) return UAPS_ERANGE;                      // labels, scores
    if (px * C * 12.0 + bc * (4.0 * kPasses * 2 * kBins + sizeof(SelState) + 8.0 * kCols) + px + 2048.0 >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}

template <int C>
void launch_col(const ColArgs& a, hipStream_t st) {
    const long groups = (long)a.B * 2 * ((a.W + 63) / 64);
    hipLaunchKernelGGL((col_kernel<C, false>), dim3((unsigned)groups), dim3(a.nseg * 64), 0, st, a);
}
}  // namespace

extern "C" int uaps_edt_workspace_bytes(int B, int H, int W, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    const int rc = check_edt(B, H, W);
    if (rc) return rc;
    *bytes = align256(2 * (size_t)B * H * W);
    return UAPS_OK;
}

extern "C" int uaps_edt_sq(const uaps_edt_call* call) {
    uaps_edt_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.mask || !c.out || !c.workspace || !dtype_ok(c.mask_dtype)) return UAPS_EINVAL;
    const int rc = check_edt(c.B, c.H, c.W);
    if (rc) return rc;
    if (c.workspace_bytes < align256(2 * (size_t)c.B * c.H * c.W)) return UAPS_EWORKSPACE;
    hipStream_t st = (hipStream_t)c.stream;
    uint16_t* g = static_cast<uint16_t*>(c.workspace);
    uaps::account_bytes((double)c.B * c.H * c.W * (c.mask_dtype + 4.0));
    ColArgs ca;
    ca.B = c.B; ca.H = c.H; ca.W = c.W; ca.nseg = segments_for(c.H); ca.esz0 = ca.esz1 = c.mask_dtype; ca.lab0 = ca.lab1 = c.mask; ca.g = g;
    hipLaunchKernelGGL((col_kernel<1, true>), dim3((unsigned)((long)c.B * ((c.W + 63) / 64))), dim3(ca.nseg * 64), 0, st, ca);
    UAPS_LAUNCH_MAIN(edt_row_kernel, dim3((unsigned)((long)c.B * c.H)), dim3(kThreads), (size_t)c.W * 4, st, (const uint16_t*)g, c.out, c.W);
    return (int)hipGetLastError();
}

extern "C" int uaps_surface_workspace_bytes(int B, int C, int H, int W, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    const int rc = check_surface(B, C, H, W);
    if (rc) return rc;
    *bytes = surface_layout(B, C, H, W).total;
    return UAPS_OK;
}

extern "C" int uaps_surface_distances(const uaps_surface_call* call) {
    uaps_surface_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.target || !c.table || !c.workspace) return UAPS_EINVAL;
    if ((c.pred != nullptr) == (c.pred_scores != nullptr)) return UAPS_EINVAL;
    if (!dtype_ok(c.target_dtype) || (c.pred && !dtype_ok(c.pred_dtype))) return UAPS_EINVAL;
    if (!(c.percentile_frac >= 0.0 && c.percentile_frac <= 1.0)) return UAPS_EINVAL;
    if ((c.has_tolerance != 0 && c.has_tolerance != 1) || c.tol_d2 < 0) return UAPS_EINVAL;
    const int rc = check_surface(c.B, c.C, c.H, c.W);
    if (rc) return rc;
    const SurfaceLayout l = surface_layout(c.B, c.C, c.H, c.W);
    if (c.workspace_bytes < l.total) return UAPS_EWORKSPACE;

    hipStream_t st = (hipStream_t)c.stream;
    char* ws = static_cast<char*>(c.workspace);
    uint16_t* g = reinterpret_cast<uint16_t*>(ws + l.g);
    int* d2 = reinterpret_cast<int*>(ws + l.d2);
    unsigned* hist = reinterpret_cast<unsigned*>(ws + l.hist);
    SelState* states = reinterpret_cast<SelState*>(ws + l.st);
    uint8_t* lab = reinterpret_cast<uint8_t*>(ws + l.lab);
    const long HW = (long)c.H * c.W, N = (long)c.B * HW;
    const int BC = c.B * c.C;
    uaps::account_bytes((double)N * ((c.pred ? (double)c.pred_dtype : 4.0 * c.C) + c.target_dtype) + 8.0 * kCols * BC);

    hipError_t e = hipMemsetAsync(c.table, 0, (size_t)BC * kCols * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(hist, 0, (size_t)BC * kPasses * 2 * kBins * 4, st);
    if (e != hipSuccess) return (int)e;
    ColArgs ca;
    ca.B = c.B; ca.H = c.H; ca.W = c.W; ca.nseg = segments_for(c.H); ca.esz0 = c.pred_dtype; ca.esz1 = c.target_dtype; ca.lab0 = c.pred; ca.lab1 = c.target; ca.g = g;
    if (c.pred_scores) {
        hipLaunchKernelGGL(argmax_kernel, dim3(grid_for(N, 1 << 20)), dim3(kThreads), 0, st, c.pred_scores, lab, c.C, HW, N);
        ca.lab0 = lab; ca.esz0 = UAPS_LABEL_U8;
    }
    switch (c.C) {
        case 1: launch_col<1>(ca, st); break;
        case 2: launch_col<2>(ca, st); break;
        case 3: launch_col<3>(ca, st); break;
        case 4: launch_col<4>(ca, st); break;
        case 5: launch_col<5>(ca, st); break;
        case 6: launch_col<6>(ca, st); break;
        case 7: launch_col<7>(ca, st); break;
        default: launch_col<8>(ca, st); break;
    }
    RowArgs ra;
    ra.H = c.H; ra.W = c.W; ra.has_tol = c.has_tolerance; ra.tol = c.tol_d2; ra.g = g; ra.d2 = d2;
    ra.table = reinterpret_cast<unsigned long long*>(c.table);
    UAPS_LAUNCH_MAIN(surface_row_kernel, dim3((unsigned)((long)BC * c.H)), dim3(kThreads), (size_t)c.W * 8, st, ra);
    hipLaunchKernelGGL(surface_ranks_kernel, dim3((BC + kThreads - 1) / kThreads), dim3(kThreads), 0, st, (long long*)c.table, states, BC,
                       c.percentile_frac);
    SelArgs sa;
    sa.HW = HW; sa.chunks = (int)((2 * HW + kChunk - 1) / kChunk); sa.d2 = d2; sa.st = states; sa.hist = hist;
    const dim3 hgrid((unsigned)((long)BC * sa.chunks)), pgrid((unsigned)BC), blk(kThreads);
    hipLaunchKernelGGL(surface_hist_kernel<0>, hgrid, blk, 0, st, sa);
    hipLaunchKernelGGL(surface_pick_kernel<0>, pgrid, blk, 0, st, states, (const unsigned*)hist, (long long*)c.table);
    hipLaunchKernelGGL(surface_hist_kernel<1>, hgrid, blk, 0, st, sa);
    hipLaunchKernelGGL(surface_pick_kernel<1>, pgrid, blk, 0, st, states, (const unsigned*)hist, (long long*)c.table);
    hipLaunchKernelGGL(surface_hist_kernel<2>, hgrid, blk, 0, st, sa);
    hipLaunchKernelGGL(surface_pick_kernel<2>, pgrid, blk, 0, st, states, (const unsigned*)hist, (long long*)c.table);
    return (int)hipGetLastError();
}
