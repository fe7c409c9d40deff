// The dense pair matrix shared by match.hip (uaps_match_instances) and detect.hip (uaps_detect_match): inter[b][p - 1][g - 1] (int32, in
// the caller's workspace) counts the pixels that carry prediction number p and ground-truth number g, both with a table row and of one
// class (or class_agnostic).  Two launches, the second after the first on one stream; integer atomics only: two runs give the same bits
// whatever order the adds arrive in.
//   zero_kernel          only the min(count_p, Mp) x min(count_g, Mg) corner of an image's matrix is ever added to or read (a label
//                        never exceeds its count): one wave per row zeroes that corner from the device-side counts; `counts` too, where
//                        the caller has a [B][C][3] table of atomically added counts (match.hip; detect.hip passes none).
//   pair_count_kernel<V> streams both label tensors once, V = 4 consecutive pixels a lane with 16-byte loads (H W % 4 == 0, aligned
//                        tensors) or V = 1.  A pixel's key is its word's offset in the matrix (it names image, p and g at once), -1
//                        where it does not count.  A lane whose V keys differ sends its own (at most V) runs; lanes of V equal keys
//                        form runs along the wave -- the run's first lane, found by comparing with the previous lane, sends ONE
//                        atomicAdd of the run's pixels, its length taken from a ballot (the scheme of instances.hip's final_kernel).
//                        Whole waves of one key are carried on in registers over the wave's kSpan groups; what a wave still carries
//                        at its end meets the other waves' in LDS, and one lane sends one atomic per distinct key of the workgroup.
//                        The sending lane does the class test: two table reads per run, not per pixel, and all of a lane's reads
//                        of one round before its adds.
// The kernels have internal linkage: every file that includes this header carries its own copy.
// Builds on call_common.hpp alone and names what it takes from it: nothing of the loss scaffold comes with this header.
#pragma once
#include "call_common.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::grid_for; using uaps::al16; using uaps::align256;

constexpr int kSpan = 4;                  // groups of 64 lanes a wave walks in pair_count_kernel

struct MatchArgs {
    int B, Mp, Mg, C, agnostic;
    long HW, N;
    double thr;
    const int* lp;                        // [B][H][W]
    const int* lg;
    const int* cnt_p;                     // [B]
    const int* cnt_g;
    const long long* tab_p;               // [B][Mp][9]
    const long long* tab_g;               // [B][Mg][9]
    int* inter;                           // [B][Mp][Mg]
    long long* out_p;                     // [B][Mp][4]
    long long* out_g;                     // [B][Mg][4]
    unsigned long long* counts;           // [B][C][3], or null
};

__device__ __forceinline__ int rows_of(const int* cnt, int b, int M) { const int n = cnt[b]; return n < 0 ? 0 : (n < M ? n : M); }

__global__ __launch_bounds__(kThreads) void zero_kernel(MatchArgs a) {
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (a.counts && t < (long)a.B * a.C * 3) a.counts[t] = 0ull;
    const int lane = threadIdx.x & 63;
    const long rows = (long)a.B * a.Mp, waves = (long)gridDim.x * kWaves;
    for (long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6); r < rows; r += waves) {
        const int b = (int)(r / a.Mp), p = (int)(r - (long)b * a.Mp);
        if (p >= rows_of(a.cnt_p, b, a.Mp)) continue;
        const int ng = rows_of(a.cnt_g, b, a.Mg);
        int* row = a.inter + r * a.Mg;
        for (int g = lane; g < ng; g += 64) row[g] = 0;
    }
}

// n pixels onto the word at offset `off` of the pair matrix, if the two components are of one class
__device__ __forceinline__ void send(const MatchArgs& a, int off, int n) {
    if (!a.agnostic) {
        const int row_p = off / a.Mg, g = off - row_p * a.Mg;          // off = (b Mp + p) Mg + g
        if (a.tab_p[(long)row_p * 9] != a.tab_g[((long)(row_p / a.Mp) * a.Mg + g) * 9]) return;
    }
    atomicAdd(a.inter + off, n);
}

// send() for the K segments of a lane (off[k] < 0: none): every class read first, then the adds, so that a lane with several segments
// waits for one round of table reads, not for one per segment
template <int K>
__device__ __forceinline__ void send_all(const MatchArgs& a, const int (&off)[K], const int (&n)[K]) {
    bool ok[K];
    if (!a.agnostic) {
        long long cp[K], cg[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            cp[k] = 0; cg[k] = 0;
            if (off[k] >= 0) {
                const int row_p = off[k] / a.Mg, g = off[k] - row_p * a.Mg;
                cp[k] = a.tab_p[(long)row_p * 9];
                cg[k] = a.tab_g[((long)(row_p / a.Mp) * a.Mg + g) * 9];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) ok[k] = off[k] >= 0 && cp[k] == cg[k];
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) ok[k] = off[k] >= 0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (ok[k]) atomicAdd(a.inter + off[k], n[k]);
}

// the last lane of the run of lanes that lane `lane` belongs to; heads = ballot of the runs' first lanes (bit 0 set)
__device__ __forceinline__ int run_end(unsigned long long heads, int lane) {
    const unsigned long long above = lane < 63 ? heads >> (lane + 1) : 0ull;
    return above ? lane + __builtin_ctzll(above) : 63;
}

template <int V>
__global__ __launch_bounds__(kThreads) void pair_count_kernel(MatchArgs a) {
    __shared__ int s_off[kWaves], s_n[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w0 = ((long)blockIdx.x * kWaves + wave) * ((long)kSpan * 64 * V);
    const int per = a.Mp * a.Mg;                     // < 2^29: the matrix stays below 2 GiB
    const long b0 = w0 / a.HW;                       // the wave's first image; the span's pixels lie less than 2^10 * V further on
    const unsigned i0 = (unsigned)(w0 - b0 * a.HW), hw = (unsigned)a.HW;
    int lp[kSpan][V], lg[kSpan][V];
#pragma unroll
    for (int it = 0; it < kSpan; ++it) {             // every load of the wave's span first
        const long n = w0 + ((long)it * 64 + lane) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) { lp[it][v] = 0; lg[it][v] = 0; }
        if (n < a.N) {                               // (V == 4: N % 4 == 0, so the four pixels are inside, and inside one image)
            if constexpr (V == 4) {
                const int4 P = *reinterpret_cast<const int4*>(a.lp + n), G = *reinterpret_cast<const int4*>(a.lg + n);
                lp[it][0] = P.x; lp[it][1] = P.y; lp[it][2] = P.z; lp[it][3] = P.w;
                lg[it][0] = G.x; lg[it][1] = G.y; lg[it][2] = G.z; lg[it][3] = G.w;
            } else {
                lp[it][0] = a.lp[n]; lg[it][0] = a.lg[n];
            }
        }
    }
    int pend_off = -1, pend_n = 0;                   // whole groups of one key, carried by the wave (uniform); lane 0 flushes
#pragma unroll
    for (int it = 0; it < kSpan; ++it) {
        const long n = w0 + ((long)it * 64 + lane) * V;
        const int base = n < a.N ? ((int)b0 + (int)((i0 + (unsigned)((it * 64 + lane) * V)) / hw)) * per : 0;
        int off[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int p = lp[it][v], g = lg[it][v];  // (0, 0 beyond the end: -1)
            off[v] = (p >= 1 && p <= a.Mp && g >= 1 && g <= a.Mg) ? base + (p - 1) * a.Mg + (g - 1) : -1;
        }
        bool same = true;
#pragma unroll
        for (int v = 1; v < V; ++v) same = same && off[v] == off[0];
        const int u = same ? off[0] : -1;            // what the lane offers to a run along the wave
        // what the lane sends in this round: slot v < V the run of its own pixels that ends at pixel v (only where its keys differ),
        // or in slot 0 the run along the wave that it heads; slot V what the wave carried and now lets go (lane 0)
        int so[V + 1], sn[V + 1];
        int len = 1;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            bool end = true;
            if (v + 1 < V) end = off[v + 1] != off[v];
            so[v] = (!same && end) ? off[v] : -1;
            sn[v] = len;
            len = end ? 1 : len + 1;
        }
        const int prev = __shfl_up(u, 1, 64);
        const bool head = lane == 0 || prev != u;
        const unsigned long long heads = __ballot(head);
        const int u0 = __shfl(u, 0, 64);
        int let_go = -1, let_go_n = pend_n;
        if (heads == 1ull && u0 >= 0) {              // the whole group is one run of one key
            if (pend_n > 0 && pend_off == u0) {
                pend_n += 64 * V;
            } else {
                if (pend_n > 0) let_go = pend_off;
                pend_off = u0; pend_n = 64 * V;
            }
        } else {
            if (pend_n > 0) let_go = pend_off;
            pend_n = 0;
            if (same && head && u >= 0) { so[0] = u; sn[0] = (run_end(heads, lane) - lane + 1) * V; }
        }
        so[V] = lane == 0 ? let_go : -1;
        sn[V] = let_go_n;
        send_all<V + 1>(a, so, sn);
    }
    // what the waves still carry: one atomic per distinct key of the workgroup (two blobs that fill the image: one key, one atomic)
    if (lane == 0) { s_off[wave] = pend_n > 0 ? pend_off : -1; s_n[wave] = pend_n; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (s_off[w] < 0) continue;
            int n = s_n[w];
#pragma unroll
            for (int x = w + 1; x < kWaves; ++x)
                if (s_off[x] == s_off[w]) { n += s_n[x]; s_off[x] = -1; }
            send(a, s_off[w], n);
        }
    }
}

// the rules of the pair matrix: 0 or the code
inline int check_matrix(int B, int Mp, int Mg) {
    if (B <= 0 || Mp <= 0 || Mg <= 0) return UAPS_EINVAL;
    if ((double)B * Mp * Mg * 4.0 >= kTooBig) return UAPS_ERANGE;
    return UAPS_OK;
}

// the two launches: `zero_waves` waves of zeroing (at least one per row of the matrix), then the count.  0, or UAPS_ERANGE (nothing
// launched) where the count's grid would not fit; the caller has checked everything else.
inline int launch_pair_count(const MatchArgs& a, long zero_waves, hipStream_t st) {
    const bool vec = a.HW % 4 == 0 && al16(a.lp) && al16(a.lg);
    const long per_block = (long)kThreads * kSpan * (vec ? 4 : 1);
    const long blocks = (a.N + per_block - 1) / per_block;  // H W < 2^31 and the label tensors of uaps_label_instances stay below 2^28 pixels
    if (blocks > 0x7FFFFFFFl) return UAPS_ERANGE;
    hipLaunchKernelGGL(zero_kernel, dim3(grid_for(zero_waves * 64, 1 << 24)), dim3(kThreads), 0, st, a);
    if (vec) UAPS_LAUNCH_MAIN(pair_count_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    else UAPS_LAUNCH_MAIN(pair_count_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    return UAPS_OK;
}
}  // namespace
