// Threshold-sweep histograms for gfx950 (include/uaps_hip.h, uaps_score_curves / uaps_plane_curves): per image and row the histogram of
// quantised scores split by a binary event -- what AUROC, AP, AUPRO, ECE and AURC are formed from on the host.  Integers throughout
// (pro_sum aside, which is summed in double in a fixed order): two runs give the same bits.
//
// Bin rule: bin(s) = clamp(floor((s - lo) * inv), 0, bins - 1), subtraction and product rounded separately in fp32 (__fsub_rn /
// __fmul_rn: no fma), the clamp in float before the conversion; a NaN enters no bin and is counted per row.
//
// A row r and an event e form a UNIT u = 2 r + e of `bins` counters; hist is [B][2 R][bins] seen that way.  Launches:
//   1 zero_kernel            hist, qsum, nan; of the region histograms only the rows below min(count[b], Mg), from the device-side count.
//   2 curves_kernel<C, V, Q> grid (B * workgroups per image, unit groups).  A workgroup of 512 threads walks kIter * 512 * V consecutive pixels of ONE
//                            image, V = 4 pixels a lane with 16-byte loads (H W % 4 == 0, aligned tensors) or V = 1.  It holds the
//                            units [u0, u0 + n) of its group as 32-bit counters in LDS (and, Q, 64-bit sums of q(s) behind them): at
//                            most 64 KB, so two workgroups fit on a CU.  units per group = floor(65536 / (bins * (Q ? 12 : 4))), at
//                            least one; the groups re-read the scores.  Per pixel and row the key is the counter's index or -1.
//                            wave_add: up to kPeel times the key of the first lane still holding one is broadcast, the lanes that
//                            hold the same key are counted with a ballot and that first lane adds ONCE; what is left after kPeel
//                            rounds (scores spread over many bins: few equal keys) is added lane by lane.  A probability map that
//                            puts nearly every pixel into the first and the last bin has at most four keys per row: no 64-fold
//                            same-address LDS atomic.  A lane whose V keys are equal sends them as one (wave-uniform test).
//                            At its end the workgroup sends the non-zero words to hist / qsum with 64-bit integer atomics.
//                            The group with a row's first unit counts its NaNs (one atomic per wave that saw one); group 0 adds,
//                            with regions, the defect pixels to region_hist: global int32 atomics through the same wave_add.
//                            C >= 2: class rows and the top row of a [B, C, H, W] score tensor (softmax in registers with
//                            from_logits); C == 1: the sigmoid head; C == 0: plane mode (one row, event pred == target).
//   3 pro_kernel             one workgroup per (image, class row): the regions of the class in ascending order, a block scan forms
//                            the suffix sums of one region, every lane adds suffix / area for its (at most 16) bins in double.  No atomics.
// Nothing waits inside a launch, no host synchronisation.
#include "loss_common.hpp"               // uaps::pixel: the logits of a pixel group, their softmax and arg-max

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::al16; using uaps::align256;

constexpr int kCT = 512;                  // threads of a curves_kernel workgroup: two waves a SIMD hide each other's wave_add chains
constexpr int kIter = 2;                  // pixel groups of kCT lanes a workgroup walks
constexpr int kPeel = 4;                  // broadcast rounds of wave_add
constexpr int kLds = 65536;               // bytes of LDS a workgroup may hold
constexpr int kMaxBins = 4096;
constexpr int kPer = kMaxBins / kThreads; // bins a lane of pro_kernel holds at most
constexpr int kMaxGrid = 1 << 16;

struct CurveArgs {
    int B, C, K, T, R, bins, from_logits, tdt, pdt, Mg, upg, wpi;   // upg: units per group, wpi: workgroups per image
    long HW;
    float lo, inv;
    int cls[UAPS_MAX_CLASSES];
    const float* S;                       // [B][C][H][W]; plane mode [B][H][W]
    const void* target;                   // [B][H][W]
    const void* pred;                     // plane mode
    const int* rl;                        // region labels [B][H][W] or NULL
    const int* rcount;                    // [B]
    const long long* rtable;              // [B][Mg][9]
    unsigned long long* hist;             // [B][2 R][bins]
    unsigned long long* qsum;             // the same or NULL
    unsigned long long* nan;              // [B][R]
    int* rhist;                           // [B][Mg][bins] (workspace)
    double* pro_sum;                      // [B][K][bins]
    long long* n_regions;                 // [B][K]
};

__device__ __forceinline__ int rows_of(const int* cnt, int b, int M) { const int n = cnt[b]; return n < 0 ? 0 : (n < M ? n : M); }

__device__ __forceinline__ int bin_of(float s, float lo, float inv, int bins) {
    float t = floorf(__fmul_rn(__fsub_rn(s, lo), inv));
    t = fminf(fmaxf(t, 0.f), (float)(bins - 1));
    return (int)t;
}

// the fixed point of instances.hip
__device__ __forceinline__ long long fixed(float v) {
    v = fminf(fmaxf(v, -65536.f), 65536.f);
    return (long long)rintf(v * 16777216.f);
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Every lane of the wave calls this (key < 0: nothing to add).  n pixels (wave-uniform) and the sum q of their q(s) go to counter `key`.
// MODE 0: LDS counters, 1: LDS counters and sums, 2: global int32 counters.
template <int MODE>
__device__ __forceinline__ void wave_add(int key, int n, long long q, unsigned* cnt, unsigned long long* qs, int* glob, int lane) {
    unsigned long long act = __ballot(key >= 0);
    for (int r = 0; r < kPeel && act; ++r) {
        const int src = __builtin_ctzll(act);
        const int lk = __builtin_amdgcn_readlane(key, src);       // (src is wave-uniform)
        const bool mine = key == lk;                       // lk >= 0
        const unsigned long long m = __ballot(mine);
        const int tot = n * __popcll(m);
        long long qt = 0;
        if constexpr (MODE == 1) {
            if (m & (m - 1)) {                             // (uniform) more than one lane: their sum
                qt = wave_sum_ll(mine ? q : 0ll);
            } else {
                const unsigned lo32 = __builtin_amdgcn_readlane((int)(unsigned)q, src), hi32 = __builtin_amdgcn_readlane((int)(q >> 32), src);
                qt = (long long)(((unsigned long long)hi32 << 32) | lo32);
            }
        }
        if (lane == src) {
            if constexpr (MODE == 2) atomicAdd(glob + lk, tot);
            else atomicAdd(cnt + lk, (unsigned)tot);
            if constexpr (MODE == 1) atomicAdd(qs + lk, (unsigned long long)qt);
        }
        if (mine) key = -1;
        act &= ~m;
    }
    if (key >= 0) {
        if constexpr (MODE == 2) atomicAdd(glob + key, n);
        else atomicAdd(cnt + key, (unsigned)n);
        if constexpr (MODE == 1) atomicAdd(qs + key, (unsigned long long)q);
    }
}

// the V keys of a lane: as one where they are equal in every lane of the wave, else one by one
template <int MODE, int V>
__device__ __forceinline__ void wave_add_v(const int (&key)[V], const long long (&q)[V], unsigned* cnt, unsigned long long* qs, int* glob,
                                           int lane) {
    bool some = false;
#pragma unroll
    for (int v = 0; v < V; ++v) some = some || key[v] >= 0;
    if (!__any(some)) return;
    if constexpr (V == 4) {
        const bool same = key[1] == key[0] && key[2] == key[0] && key[3] == key[0];
        if (__all(same)) {
            wave_add<MODE>(key[0], 4, (q[0] + q[1]) + (q[2] + q[3]), cnt, qs, glob, lane);
            return;
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) wave_add<MODE>(key[v], 1, q[v], cnt, qs, glob, lane);
}

// V consecutive labels of element size esz (UAPS_LABEL_*)
template <int V>
__device__ __forceinline__ void load_any_labels(const void* __restrict__ p, long n, int esz, long long (&t)[V]) {
    if constexpr (V == 4) {
        if (esz == 8) {
            const long long* q = static_cast<const long long*>(p) + n;
            const longlong2 a = *reinterpret_cast<const longlong2*>(q), b = *reinterpret_cast<const longlong2*>(q + 2);
            t[0] = a.x; t[1] = a.y; t[2] = b.x; t[3] = b.y;
        } else if (esz == 4) {
            const int4 a = *reinterpret_cast<const int4*>(static_cast<const int*>(p) + n);
            t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
        } else {
            const uchar4 a = *reinterpret_cast<const uchar4*>(static_cast<const uint8_t*>(p) + n);
            t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
        }
    } else {
        if (esz == 8) t[0] = static_cast<const long long*>(p)[n];
        else if (esz == 4) t[0] = static_cast<const int*>(p)[n];
        else t[0] = static_cast<const uint8_t*>(p)[n];
    }
}

// n NaN pixels of this lane onto nan[row]: one atomic per wave that saw one
__device__ __forceinline__ void count_nan(unsigned long long* word, int n, int lane) {
    if (!__any(n > 0)) return;
    int tot = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    if (lane == 0) atomicAdd(word, (unsigned long long)tot);
}

template <int C, int V, bool Q>
__global__ __launch_bounds__(kCT) void curves_kernel(CurveArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int CC = C > 0 ? C : 1;
    constexpr int MODE = Q ? 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int U = 2 * a.R;
    const int u0 = (int)blockIdx.y * a.upg;
    const int nu = (U - u0) < a.upg ? (U - u0) : a.upg;
    const int cells = nu * a.bins;
    unsigned* cnt = reinterpret_cast<unsigned*>(smem);
    // the sums start on the next multiple of 8 bytes behind the counters (upg and bins may both be odd)
    unsigned long long* qs = reinterpret_cast<unsigned long long*>(smem + (((size_t)a.upg * a.bins * 4 + 7) & ~(size_t)7));
    for (int i = tid; i < cells; i += kCT) {
        cnt[i] = 0u;
        if constexpr (Q) qs[i] = 0ull;
    }
    __syncthreads();
    const int b = (int)blockIdx.x / a.wpi, chunk = (int)blockIdx.x - b * a.wpi;
    const long first = (long)chunk * (kCT * V * kIter);
    const bool lead = blockIdx.y == 0;                       // the group that fills the region histograms
    const int k_lo = u0 >> 1, k_hi = (u0 + nu + 1) >> 1;     // the rows with a unit in [u0, u0 + nu)
    const bool logits = a.from_logits != 0;

    for (int it = 0; it < kIter; ++it) {
        if (first + (long)it * (kCT * V) >= a.HW) break;                      // (uniform)
        const long i = first + ((long)it * kCT + tid) * V;
        const bool in = i < a.HW;                            // (V == 4: H W % 4 == 0, so the four pixels are inside)
        float z[CC][V];
        float raw[V];                                        // C == 1: the logit
        long long t[V], pr[V];
        int g[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            t[v] = -1; pr[v] = 0; g[v] = 0; raw[v] = 0.f;
#pragma unroll
            for (int c = 0; c < CC; ++c) z[c][v] = 0.f;
        }
        if (in) {
            const long px = (long)b * a.HW + i;
            uaps::pixel::load_logits<CC, V>(a.S + (long)b * CC * a.HW + i, a.HW, z);
            load_any_labels<V>(a.target, px, a.tdt, t);
            if constexpr (C == 0) load_any_labels<V>(a.pred, px, a.pdt, pr);
            if (C > 0 && lead && a.rl) {
                if constexpr (V == 4) {
                    const int4 G = *reinterpret_cast<const int4*>(a.rl + px);
                    g[0] = G.x; g[1] = G.y; g[2] = G.z; g[3] = G.w;
                } else {
                    g[0] = a.rl[px];
                }
            }
        }
        // the pixel's class (-1: ignored), its top-row prediction, whether any of its scores is NaN
        int y[V], am[V];
        bool bad[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            am[v] = 0;
            if constexpr (C == 0) y[v] = t[v] >= 0 ? 1 : -1;
            else if constexpr (C == 1) y[v] = (t[v] == 0 || t[v] == 1) ? (int)t[v] : -1;
            else y[v] = (t[v] >= 0 && t[v] < C) ? (int)t[v] : -1;
        }
        if constexpr (C >= 2) {
            uaps::pixel::argmax_logits<C, V>(z, am);        // on the logits with from_logits, as everywhere else
            if (logits) {
                float mx[V], lse[V];
                uaps::pixel::softmax_inplace<C, V>(z, mx, lse);
            }
        }
        if constexpr (C == 1) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                raw[v] = z[0][v];
                if (logits) { z[0][v] = 1.f / (1.f + expf(-raw[v])); am[v] = raw[v] > 0.f ? 1 : 0; }
                else am[v] = raw[v] > 0.5f ? 1 : 0;
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            bad[v] = false;
#pragma unroll
            for (int c = 0; c < CC; ++c) bad[v] = bad[v] || (z[c][v] != z[c][v]);
        }

        for (int k = k_lo; k < k_hi; ++k) {                  // (uniform)
            int key[V];
            long long q[V];
            int nn = 0;
            const bool top = k >= a.K;                       // plane mode: K = 1, T = 0
            const int c = top ? 0 : a.cls[k];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float s;
                bool ev, isn;
                if constexpr (C == 0) {
                    s = z[0][v]; ev = pr[v] == t[v]; isn = bad[v];
                } else if constexpr (C == 1) {
                    if (top) { s = fmaxf(z[0][v], __fsub_rn(1.f, z[0][v])); ev = am[v] == y[v]; }
                    else { s = z[0][v]; ev = y[v] == 1; }
                    isn = bad[v];
                } else {
                    if (top) {
                        s = z[0][v];
#pragma unroll
                        for (int cc = 1; cc < C; ++cc) s = z[cc][v] > s ? z[cc][v] : s;
                        ev = am[v] == y[v]; isn = bad[v];
                    } else {
                        s = uaps::pixel::pick<C, V>(z, v, c); ev = y[v] == c; isn = s != s;
                    }
                }
                const int u = 2 * k + (ev ? 1 : 0) - u0;
                const bool ok = y[v] >= 0;
                nn += (ok && isn) ? 1 : 0;
                key[v] = (ok && !isn && u >= 0 && u < nu) ? u * a.bins + bin_of(s, a.lo, a.inv, a.bins) : -1;
                q[v] = 0;
                if constexpr (Q) q[v] = isn ? 0ll : fixed(s);
            }
            if (2 * k >= u0) count_nan(a.nan + (long)b * a.R + k, nn, lane);        // the group that holds the row's first unit
            wave_add_v<MODE, V>(key, q, cnt, qs, nullptr, lane);
        }

        if (C > 0 && lead && a.rl) {                         // (uniform)
            int key[V];
            long long q[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                key[v] = -1; q[v] = 0;
                if (g[v] >= 1 && g[v] <= a.Mg) {
                    const int row = b * a.Mg + g[v] - 1;
                    const long long rc = a.rtable[(long)row * 9];
                    float s = 0.f;
                    bool ok;
                    if constexpr (C == 1) { ok = rc == 1; s = z[0][v]; }
                    else { ok = rc >= 0 && rc < CC; s = uaps::pixel::pick<CC, V>(z, v, (int)rc); }
                    if (ok && s == s) key[v] = row * a.bins + bin_of(s, a.lo, a.inv, a.bins);     // below 2^29: the workspace stays below 2 GiB
                }
            }
            wave_add_v<2, V>(key, q, nullptr, nullptr, a.rhist, lane);
        }
    }

    __syncthreads();
    const long out0 = ((long)b * U + u0) * a.bins;
    for (int i = tid; i < cells; i += kCT) {
        const unsigned n = cnt[i];
        if (n) atomicAdd(a.hist + out0 + i, (unsigned long long)n);
        if constexpr (Q) {
            const unsigned long long s = qs[i];
            if (s) atomicAdd(a.qsum + out0 + i, s);
        }
    }
}

__global__ __launch_bounds__(kThreads) void zero_kernel(CurveArgs a) {
    const long n_hist = (long)a.B * a.R * 2 * a.bins, n_nan = (long)a.B * a.R;
    const long step = (long)gridDim.x * kThreads;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n_hist; i += step) {
        a.hist[i] = 0ull;
        if (a.qsum) a.qsum[i] = 0ull;
        if (i < n_nan) a.nan[i] = 0ull;
    }
    if (!a.rl) return;
    const int lane = threadIdx.x & 63;
    const long rows = (long)a.B * a.Mg, waves = (long)gridDim.x * kWaves;
    for (long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); r < rows; r += waves) {
        const int b = (int)(r / a.Mg), g = (int)(r - (long)b * a.Mg);
        if (g >= rows_of(a.rcount, b, a.Mg)) continue;
        int* row = a.rhist + r * a.bins;
        for (int i = lane; i < a.bins; i += 64) row[i] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void pro_kernel(CurveArgs a) {
    __shared__ long long s_w[kWaves];
    const int b = (int)blockIdx.x / a.K, k = (int)blockIdx.x - b * a.K;
    const int c = a.cls[k];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (a.bins + kThreads - 1) / kThreads;      // <= kPer
    const int nr = rows_of(a.rcount, b, a.Mg);
    double acc[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) acc[j] = 0.0;
    long long count = 0;
    for (int r = 0; r < nr; ++r) {                           // ascending: the order of the double sums
        const long long* row = a.rtable + ((long)b * a.Mg + r) * 9;
        const long long area = row[1];
        if (row[0] != c || area <= 0) continue;              // (uniform)
        ++count;
        const int* h = a.rhist + ((long)b * a.Mg + r) * a.bins;
        int v[kPer];
        long long tot = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int bin = t * per + j;
            v[j] = (j < per && bin < a.bins) ? h[bin] : 0;
            tot += v[j];
        }
        long long incl = tot;                                // the sum over the lanes from this one on
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long x = __shfl_down(incl, o, 64);
            if (lane + o < 64) incl += x;
        }
        __syncthreads();                                     // s_w is reused by the next region
        if (lane == 0) s_w[wave] = incl;
        __syncthreads();
#pragma unroll
        for (int w = 1; w < kWaves; ++w)
            if (w > wave) incl += s_w[w];
        long long s = incl - tot;                            // the bins behind this lane's
        const double d_area = (double)area;
#pragma unroll
        for (int j = kPer - 1; j >= 0; --j) {
            s += v[j];
            if (j < per) acc[j] += (double)s / d_area;
        }
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int bin = t * per + j;
        if (j < per && bin < a.bins) a.pro_sum[((long)b * a.K + k) * a.bins + bin] = acc[j];
    }
    if (t == 0) a.n_regions[(long)b * a.K + k] = count;
}

inline bool dtype_ok(int d) { return d == UAPS_LABEL_U8 || d == UAPS_LABEL_I32 || d == UAPS_LABEL_I64; }
inline bool finite_f(float v) { return v - v == 0.f; }

// units per group and the bytes of LDS a workgroup then holds
inline int units_per_group(int R, int bins, bool q) {
    const int cell = q ? 12 : 4;
    int u = kLds / (bins * cell);
    u = u < 1 ? 1 : u;
    return u > 2 * R ? 2 * R : u;
}

template <int C, int V>
void launch_q(bool q, dim3 grid, size_t lds, hipStream_t st, const CurveArgs& a) {
    if (q) UAPS_LAUNCH_MAIN((curves_kernel<C, V, true>), grid, dim3(kCT), lds, st, a);
    else UAPS_LAUNCH_MAIN((curves_kernel<C, V, false>), grid, dim3(kCT), lds, st, a);
}
template <int C>
void launch_v(bool vec, bool q, dim3 grid, size_t lds, hipStream_t st, const CurveArgs& a) {
    if (vec) launch_q<C, 4>(q, grid, lds, st, a);
    else launch_q<C, 1>(q, grid, lds, st, a);
}

// zero, the histogram pass and, with regions, the reduction
int run(CurveArgs& a, bool vec, hipStream_t st) {
    const bool q = a.qsum != nullptr;
    a.upg = units_per_group(a.R, a.bins, q);
    const int groups = (2 * a.R + a.upg - 1) / a.upg;
    // counters, rounded up to 8 bytes, then the 64-bit sums: odd * odd * 12 is at most 65532, so the four bytes still fit in kLds
    const size_t counters = ((size_t)a.upg * a.bins * 4 + 7) & ~(size_t)7;
    const size_t lds = q ? counters + (size_t)a.upg * a.bins * 8 : (size_t)a.upg * a.bins * 4;
    const long span = (long)kCT * kIter * (vec ? 4 : 1);
    a.wpi = (int)((a.HW + span - 1) / span);
    const long blocks = (long)a.B * a.wpi;                   // H W < 2^31 and B H W 4 < 2^31: below 2^20
    if (blocks > 0x7FFFFFFFl || groups > 65535) return UAPS_ERANGE;
    long zero_items = (long)a.B * a.R * 2 * a.bins;
    if (a.rl && (long)a.B * a.Mg * 64 > zero_items) zero_items = (long)a.B * a.Mg * 64;
    hipLaunchKernelGGL(zero_kernel, dim3(grid_for(zero_items, kMaxGrid)), dim3(kThreads), 0, st, a);
    const dim3 grid((unsigned)blocks, (unsigned)groups);
    switch (a.C) {
        case 0: launch_v<0>(vec, q, grid, lds, st, a); break;
        case 1: launch_v<1>(vec, q, grid, lds, st, a); break;
        case 2: launch_v<2>(vec, q, grid, lds, st, a); break;
        case 3: launch_v<3>(vec, q, grid, lds, st, a); break;
        case 4: launch_v<4>(vec, q, grid, lds, st, a); break;
        case 5: launch_v<5>(vec, q, grid, lds, st, a); break;
        case 6: launch_v<6>(vec, q, grid, lds, st, a); break;
        case 7: launch_v<7>(vec, q, grid, lds, st, a); break;
        case 8: launch_v<8>(vec, q, grid, lds, st, a); break;
        default: return UAPS_ERANGE;
    }
    if (a.rl && a.K > 0) hipLaunchKernelGGL(pro_kernel, dim3((unsigned)(a.B * a.K)), dim3(kThreads), 0, st, a);
    return (int)hipGetLastError();
}

// bins, the range and the derived factor: 0 or the code
inline int check_range(int bins, float lo, float hi, float* inv) {
    if (!finite_f(lo) || !finite_f(hi) || !(lo < hi)) return UAPS_EINVAL;
    if (bins < 2 || bins > kMaxBins) return UAPS_ERANGE;
    *inv = (float)bins / (hi - lo);                          // fp32, once, here
    if (!finite_f(*inv) || !(*inv > 0.f)) return UAPS_EINVAL;
    return UAPS_OK;
}
}  // namespace

extern "C" int uaps_curves_workspace_bytes(int B, int max_regions, int bins, size_t* bytes) {
    if (!bytes || B <= 0 || max_regions < 0) return UAPS_EINVAL;
    if (bins < 2 || bins > kMaxBins) return UAPS_ERANGE;
    if (4.0 * (double)B * max_regions * bins >= kTooBig) return UAPS_ERANGE;
    *bytes = align256(4 * (size_t)B * max_regions * bins);
    return UAPS_OK;
}

extern "C" int uaps_score_curves(const uaps_curves_call* call) {
    uaps_curves_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.scores || !c.target || !c.hist || !c.nan) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0) return UAPS_EINVAL;
    if ((c.from_logits != 0 && c.from_logits != 1) || (c.top_row != 0 && c.top_row != 1)) return UAPS_EINVAL;
    if (!dtype_ok(c.target_dtype)) return UAPS_EINVAL;
    if (c.n_classes < 0 || c.n_classes > UAPS_MAX_CLASSES || c.n_classes + c.top_row == 0) return UAPS_EINVAL;
    const bool regions = c.region_labels || c.region_count || c.region_table || c.pro_sum || c.n_regions || c.max_regions != 0;
    if (regions && (!c.region_labels || !c.region_count || !c.region_table || !c.pro_sum || !c.n_regions || c.max_regions <= 0))
        return UAPS_EINVAL;
    if (c.C < 1 || c.C > UAPS_MAX_CLASSES) return UAPS_ERANGE;
    for (int k = 0; k < c.n_classes; ++k) {                  // the sigmoid head scores class 1
        if (c.C == 1 ? c.classes[k] != 1 : (c.classes[k] < 0 || c.classes[k] >= c.C)) return UAPS_EINVAL;
    }
    float inv = 0.f;
    const int rc = check_range(c.bins, c.lo, c.hi, &inv);
    if (rc) return rc;
    const double HW = (double)c.H * c.W;
    const int R = c.n_classes + c.top_row;
    if (HW >= kTooBig || HW * c.B * c.C * 4.0 >= kTooBig || HW * c.B * c.target_dtype >= kTooBig) return UAPS_ERANGE;
    if ((double)c.B * R * 2.0 * c.bins * 8.0 >= kTooBig) return UAPS_ERANGE;
    size_t need = 0;
    if (regions) {
        if ((double)c.B * c.max_regions * 72.0 >= kTooBig || 4.0 * (double)c.B * c.max_regions * c.bins >= kTooBig) return UAPS_ERANGE;
        need = align256(4 * (size_t)c.B * c.max_regions * c.bins);
        if (!c.workspace || !uaps::workspace_ok(c.workspace, c.workspace_bytes, need)) return UAPS_EINVAL;
    }

    CurveArgs a;
    memset(&a, 0, sizeof a);
    a.B = c.B; a.C = c.C; a.K = c.n_classes; a.T = c.top_row; a.R = R; a.bins = c.bins; a.from_logits = c.from_logits;
    a.tdt = c.target_dtype; a.pdt = c.target_dtype; a.Mg = regions ? c.max_regions : 0;
    a.HW = (long)c.H * c.W; a.lo = c.lo; a.inv = inv;
    for (int k = 0; k < c.n_classes; ++k) a.cls[k] = c.classes[k];
    a.S = c.scores; a.target = c.target; a.pred = nullptr;
    a.rl = regions ? c.region_labels : nullptr; a.rcount = c.region_count; a.rtable = (const long long*)c.region_table;
    a.hist = (unsigned long long*)c.hist; a.qsum = (unsigned long long*)c.qsum; a.nan = (unsigned long long*)c.nan;
    a.rhist = static_cast<int*>(c.workspace); a.pro_sum = c.pro_sum; a.n_regions = (long long*)c.n_regions;
    const bool vec = a.HW % 4 == 0 && al16(a.S) && al16(a.target) && (!a.rl || al16(a.rl));
    uaps::account_bytes((double)c.B * HW * (4.0 * c.C + c.target_dtype + (regions ? 4.0 : 0.0)) +
                        (double)c.B * R * c.bins * (c.qsum ? 32.0 : 16.0));
    return run(a, vec, (hipStream_t)c.stream);
}

extern "C" int uaps_plane_curves(const uaps_plane_curves_call* call) {
    uaps_plane_curves_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.score || !c.pred || !c.target || !c.hist || !c.nan) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0) return UAPS_EINVAL;
    if (c.from_logits != 0) return UAPS_EINVAL;              // a plane is no class probability: nothing to form a softmax over
    if (!dtype_ok(c.pred_dtype) || !dtype_ok(c.target_dtype)) return UAPS_EINVAL;
    float inv = 0.f;
    const int rc = check_range(c.bins, c.lo, c.hi, &inv);
    if (rc) return rc;
    const double HW = (double)c.H * c.W;
    if (HW >= kTooBig || HW * c.B * 4.0 >= kTooBig || HW * c.B * c.target_dtype >= kTooBig || HW * c.B * c.pred_dtype >= kTooBig)
        return UAPS_ERANGE;
    if ((double)c.B * 2.0 * c.bins * 8.0 >= kTooBig) return UAPS_ERANGE;

    CurveArgs a;
    memset(&a, 0, sizeof a);
    a.B = c.B; a.C = 0; a.K = 1; a.T = 0; a.R = 1; a.bins = c.bins; a.tdt = c.target_dtype; a.pdt = c.pred_dtype;
    a.HW = (long)c.H * c.W; a.lo = c.lo; a.inv = inv;
    a.S = c.score; a.target = c.target; a.pred = c.pred;
    a.hist = (unsigned long long*)c.hist; a.qsum = (unsigned long long*)c.qsum; a.nan = (unsigned long long*)c.nan;
    const bool vec = a.HW % 4 == 0 && al16(a.S) && al16(a.target) && al16(a.pred);
    uaps::account_bytes((double)c.B * HW * (4.0 + c.target_dtype + c.pred_dtype) + (double)c.B * c.bins * (c.qsum ? 32.0 : 16.0));
    return run(a, vec, (hipStream_t)c.stream);
}
