// Defect detection matching over an IoU sweep for gfx950 (include/uaps_hip.h, uaps_detect_match): COCO's greedy assignment of scored
// detections to ground-truth defects at T thresholds at once, on the pair matrix of match.hip (pair_count.hpp).  DESIGN.md 3.31.
//
// Five launches on one stream, every one a coherence point for the next; integer atomics only in the pair count, no workgroup waits
// for another, every later word has one writer: two runs give the same bits.
//   1 zero_kernel, 2 pair_count_kernel<V>   pair_count.hpp
//   3 candidates_kernel   one wave per (b, p) scans its row of `inter` once and keeps the g that pass the IoU test at the LOWEST
//                         threshold: inter >= t_min union >= t_min area_p, and the ground-truth defects are disjoint, so at most
//                         floor(1000 / t1000_min) <= 10 pass -- a fixed-size list (g, inter, union), no overflow path (a slot guard
//                         covers tables that contradict their label map).  The wave orders the list by (IoU descending, g ascending)
//                         with the exact 64-bit cross-multiplication, one lane per entry counting the entries before its own, and
//                         stores with every entry the number of thresholds it passes (1000 inter >= t1000 union; the thresholds
//                         ascend, so it passes exactly the first npass).  The same launch forms the score key and zeroes the row's
//                         pred_match / pred_inter.
//   4 order_kernel        one workgroup per image: the keys (a monotone map of the float64 bits, NaN lowest) and classes staged in LDS,
//                         rank[p] = #{q of p's class: key_q > key_p, or equal and q < p}; position = #{q of a lower class} + rank gives
//                         the class-major sequence.  n_pred (from the class size the same loop counts) and n_gt (a barrier count per
//                         class) go to `counts` through LDS, tp zeroed; target_match zeroed.
//   5 sweep_kernel        the sequential part: one wave per image, LANE = THRESHOLD.  The sequence is read 64 detections at a time, the
//                         candidate lists of those with any are staged in LDS, and for each in turn lane t walks the list while
//                         t < npass and takes the first g whose bit in its own taken-mask (LDS, word-major so that the
//                         lanes hit distinct banks) is clear.  The list is in (IoU descending, g ascending) order and passing is monotone
//                         along it, so this is the literal greedy rule.  tp is carried in a register and stored at a class change.
#include "pair_count.hpp"

namespace {
constexpr int kMaxT = UAPS_DETECT_MAX_THRESHOLDS;
constexpr int kMaxCand = UAPS_DETECT_MAX_CANDIDATES;
constexpr int kMaxRows = UAPS_DETECT_MAX_ROWS;
constexpr int kOrderThreads = 1024;
constexpr int kPer = kMaxRows / kOrderThreads;      // table rows a thread of order_kernel holds
constexpr int kScan = 4;                            // row words a lane of candidates_kernel reads before it tests
using uaps::u64;

struct DetArgs {
    MatchArgs m;                                    // B, Mp, Mg, C, agnostic, counts, tables and the pair matrix
    int T, max_dets;
    int t1000[kMaxT];
    const double* scores;                           // [B][Mp] or null
    double* score;                                  // [B][Mp]
    long long* rank;                                // [B][Mp]
    long long* pred_match;                          // [B][Mp][T]
    long long* pred_inter;                          // [B][Mp][T]
    long long* target_match;                        // [B][Mg][T]
    long long* counts;                              // [B][C][T + 2]
    int4* cand;                                     // [B][Mp][kMaxCand]: g, inter, union, the number of thresholds the pair passes
    int* ncand;                                     // [B][Mp]
    u64* key;                                       // [B][Mp]
    int2* seq;                                      // [B][Mp]: (row p or -1 where max_dets cuts it, class), class-major in rank order
    int* nseq;                                      // [B]
};

// a before b in a detection's list: the larger IoU, the lower number on ties (inter_a / union_a > inter_b / union_b, exactly)
__device__ __forceinline__ bool better(const int4& a, const int4& b) {
    const long long l = (long long)a.y * b.z, r = (long long)b.y * a.z;
    return l > r || (l == r && a.x < b.x);
}

__global__ __launch_bounds__(kThreads) void candidates_kernel(DetArgs d) {
    __shared__ int4 s_list[kWaves][kMaxCand];
    const MatchArgs& a = d.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * kWaves + wave;
    const bool live = r < (long)a.B * a.Mp;                                    // (wave-uniform, like `has`)
    const int b = live ? (int)(r / a.Mp) : 0, p = live ? (int)(r - (long)b * a.Mp) : 0;
    const bool has = live && p < rows_of(a.cnt_p, b, a.Mp);
    int n = 0;
    long long area_p = 0;
    if (has) {
        area_p = a.tab_p[r * 9 + 1];
        const int ng = rows_of(a.cnt_g, b, a.Mg);
        const int* row = a.inter + r * a.Mg;
        const long long tmin = d.t1000[0];
        for (int g0 = 0; g0 < ng; g0 += 64 * kScan) {
            int v[kScan];
#pragma unroll
            for (int k = 0; k < kScan; ++k) {
                const int g = g0 + k * 64 + lane;
                v[k] = g < ng ? row[g] : 0;
            }
#pragma unroll
            for (int k = 0; k < kScan; ++k) {
                const int g = g0 + k * 64 + lane;
                bool pass = false;
                long long uni = 0;
                if (v[k] > 0) {
                    uni = area_p + a.tab_g[((long)b * a.Mg + g) * 9 + 1] - v[k];
                    pass = uni > 0 && uni <= 0x7FFFFFFFll && 1000ll * v[k] >= tmin * uni;
                }
                const u64 mask = __ballot(pass);
                if (pass) {
                    const int slot = n + __popcll(mask & ((1ull << lane) - 1ull));
                    if (slot < kMaxCand) s_list[wave][slot] = make_int4(g + 1, v[k], (int)uni, 0);
                }
                n += __popcll(mask);
            }
        }
        n = n < kMaxCand ? n : kMaxCand;
    }
    __syncthreads();
    if (!live) return;
    if (lane < n) {
        int4 mine = s_list[wave][lane];
        int pos = 0;
        for (int j = 0; j < n; ++j) pos += better(s_list[wave][j], mine) ? 1 : 0;
        int npass = 0;                                                         // the thresholds ascend: the pair passes exactly the first npass
#pragma unroll
        for (int t = 0; t < kMaxT; ++t) npass += (t < d.T && 1000ll * mine.y >= (long long)d.t1000[t] * mine.z) ? 1 : 0;
        mine.w = npass;
        d.cand[r * kMaxCand + pos] = mine;
    }
    if (lane < d.T) {
        d.pred_match[r * d.T + lane] = 0;
        d.pred_inter[r * d.T + lane] = 0;
    }
    if (lane != 0) return;
    d.ncand[r] = n;
    double s = -__builtin_inf();
    u64 key = 0ull;                                                            // NaN: after every number
    if (has) {
        const double x = d.scores ? d.scores[r] : __ddiv_rn((double)a.tab_p[r * 9 + 7], (double)area_p);
        if (x == x) {
            s = x + 0.0;                                                       // -0 -> +0
            const long long bits = __double_as_longlong(s);
            key = bits < 0 ? ~(u64)bits : ((u64)bits | 0x8000000000000000ull);
        }
    }
    d.score[r] = s;
    d.key[r] = key;
}

// the counting loop of order_kernel for the first J rows of a thread: every q is one broadcast read of its class and key (no branch on
// them, eight q in flight), same = #{q of the row's class}, before = those ordered before it, lower = #{q of a lower class}
template <int J>
__device__ __forceinline__ void count_before(const u64* s_key, const int* s_cls, int np, int tid, const u64 (&k)[kPer], const int (&c)[kPer],
                                             int (&before)[kPer], int (&lower)[kPer], int (&same)[kPer]) {
#pragma unroll 8
    for (int q = 0; q < np; ++q) {
        const int cq = s_cls[q];
        const u64 kq = s_key[q];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int p = tid + j * kOrderThreads;
            const bool eq = cq >= 0 && cq == c[j];
            same[j] += eq ? 1 : 0;
            before[j] += (eq && (kq > k[j] || (kq == k[j] && q < p))) ? 1 : 0;
            lower[j] += (cq >= 0 && cq < c[j]) ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(kOrderThreads) void order_kernel(DetArgs d) {
    __shared__ u64 s_key[kMaxRows];
    __shared__ int s_cls[kMaxRows];
    __shared__ int s_cnt[UAPS_MATCH_MAX_CLASSES][2];                           // n_pred taking part, n_gt
    const MatchArgs& a = d.m;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int np = rows_of(a.cnt_p, b, a.Mp), ng = rows_of(a.cnt_g, b, a.Mg);
    const int maxd = d.max_dets > 0 ? d.max_dets : 0x7FFFFFFF;
    for (int p = tid; p < np; p += kOrderThreads) {
        s_key[p] = d.key[(long)b * a.Mp + p];
        const long long cls = a.agnostic ? 0 : a.tab_p[((long)b * a.Mp + p) * 9];
        s_cls[p] = (cls >= 0 && cls < a.C) ? (int)cls : -1;
    }
    for (int i = tid; i < a.C * 2; i += kOrderThreads) s_cnt[i >> 1][i & 1] = 0;
    long long* tm = d.target_match + (long)b * a.Mg * d.T;
    for (int i = tid; i < a.Mg * d.T; i += kOrderThreads) tm[i] = 0;
    __syncthreads();
    u64 k[kPer];
    int c[kPer], before[kPer], lower[kPer], same[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int p = tid + j * kOrderThreads;
        k[j] = p < np ? s_key[p] : 0ull;
        c[j] = p < np ? s_cls[p] : -1;
        before[j] = 0; lower[j] = 0; same[j] = 0;
    }
    const int nper = (np + kOrderThreads - 1) / kOrderThreads;                 // (uniform)
    if (tid - (tid & 63) >= np) {}                                             // a wave without a row has nothing to count
    else if (nper <= 1) count_before<1>(s_key, s_cls, np, tid, k, c, before, lower, same);
    else if (nper == 2) count_before<2>(s_key, s_cls, np, tid, k, c, before, lower, same);
    else count_before<kPer>(s_key, s_cls, np, tid, k, c, before, lower, same);
    int total = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int p = tid + j * kOrderThreads;
        const bool in = c[j] >= 0;                                             // (p < np)
        if (in) {
            const bool part = before[j] < maxd;
            d.rank[(long)b * a.Mp + p] = part ? before[j] : -1;
            d.seq[(long)b * a.Mp + lower[j] + before[j]] = make_int2(part ? p : -1, c[j]);
            if (before[j] == 0) s_cnt[c[j]][0] = same[j] < maxd ? same[j] : maxd;
        } else if (p < a.Mp) {
            d.rank[(long)b * a.Mp + p] = -1;
        }
        total += __syncthreads_count(in ? 1 : 0);
    }
    if (tid == 0) d.nseq[b] = total;
    // n_gt per class: a barrier count per class and group of kOrderThreads rows
    if (a.agnostic) {
        if (tid == 0) s_cnt[0][1] = ng;
    } else {
        int cg[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int g = tid + j * kOrderThreads;
            long long cls = -1;
            if (g < ng) cls = a.tab_g[((long)b * a.Mg + g) * 9];
            cg[j] = (cls >= 0 && cls < a.C) ? (int)cls : -1;
        }
        const int gper = (ng + kOrderThreads - 1) / kOrderThreads;
        for (int cl = 0; cl < a.C; ++cl) {
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < kPer; ++j)
                if (j < gper) cnt += __syncthreads_count(cg[j] == cl ? 1 : 0);
            if (tid == 0) s_cnt[cl][1] = cnt;
        }
    }
    __syncthreads();
    long long* out = d.counts + (long)b * a.C * (d.T + 2);
    for (int i = tid; i < a.C * (d.T + 2); i += kOrderThreads) {
        const int cl = i / (d.T + 2), t = i - cl * (d.T + 2);
        out[i] = t < d.T ? 0 : s_cnt[cl][t - d.T];
    }
}

__global__ __launch_bounds__(64) void sweep_kernel(DetArgs d) {
    __shared__ unsigned s_taken[(kMaxRows / 32) * 32];                         // [word of 32 ground-truth numbers][threshold]
    __shared__ int4 s_list[64][kMaxCand];
    const MatchArgs& a = d.m;
    const int b = blockIdx.x, lane = threadIdx.x, T = d.T;
    const int ng = rows_of(a.cnt_g, b, a.Mg);
    for (int i = lane; i < ((ng + 31) >> 5) * 32; i += 64) s_taken[i] = 0u;
    __syncthreads();
    const int nseq = d.nseq[b];
    const long row0 = (long)b * a.Mp;
    long long* counts = d.counts + (long)b * a.C * (T + 2);
    long long tp = 0;
    int cur = -1;
    for (int base = 0; base < nseq; base += 64) {
        int2 e = make_int2(-1, -1);
        if (base + lane < nseq) e = d.seq[row0 + base + lane];
        const int p = e.x;
        const int n = p >= 0 ? d.ncand[row0 + p] : 0;
        u64 todo = __ballot(n > 0);
        if (!todo) continue;                                                   // (uniform)
#pragma unroll
        for (int it = 0; it < kMaxCand; ++it) {                                // the 64 lists, every load before the first use
            const int idx = it * 64 + lane, j = idx / kMaxCand, k = idx - j * kMaxCand;
            const int pj = __shfl(p, j, 64), nj = __shfl(n, j, 64);
            if (k < nj) s_list[j][k] = d.cand[(row0 + pj) * kMaxCand + k];
        }
        __syncthreads();
        while (todo) {
            const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));        // (uniform: todo is a ballot)
            todo &= todo - 1ull;
            const int pj = __builtin_amdgcn_readlane(p, j), nj = __builtin_amdgcn_readlane(n, j), cj = __builtin_amdgcn_readlane(e.y, j);
            if (cj != cur) {
                if (cur >= 0 && lane < T) counts[cur * (T + 2) + lane] = tp;
                tp = 0;
                cur = cj;
            }
            if (lane < T) {
                for (int k = 0; k < nj; ++k) {
                    const int4 c = s_list[j][k];
                    if (lane >= c.w) break;                                    // fails this threshold; the list is in IoU order: so does the rest
                    const int w = ((c.x - 1) >> 5) * 32 + lane;
                    const unsigned bit = 1u << ((c.x - 1) & 31), m = s_taken[w];
                    if (!(m & bit)) {
                        s_taken[w] = m | bit;
                        d.pred_match[(row0 + pj) * T + lane] = c.x;
                        d.pred_inter[(row0 + pj) * T + lane] = c.y;
                        d.target_match[((long)b * a.Mg + c.x - 1) * T + lane] = pj + 1;
                        ++tp;
                        break;
                    }
                }
            }
        }
        __syncthreads();                                                       // the next group overwrites the lists
    }
    if (cur >= 0 && lane < T) counts[cur * (T + 2) + lane] = tp;
}

struct Layout { size_t inter, cand, ncand, key, seq, nseq, total; };

inline Layout layout(int B, int Mp, int Mg) {
    const size_t rows = (size_t)B * Mp;
    Layout l;
    l.inter = 0;
    l.cand = align256(4 * rows * Mg);
    l.ncand = l.cand + align256(sizeof(int4) * kMaxCand * rows);
    l.key = l.ncand + align256(4 * rows);
    l.seq = l.key + align256(8 * rows);
    l.nseq = l.seq + align256(8 * rows);
    l.total = l.nseq + align256(4 * (size_t)B);
    return l;
}

// the size rules: 0 or the code
inline int check_sizes(int B, int Mp, int Mg, int T) {
    const int rc = check_matrix(B, Mp, Mg);
    if (rc == UAPS_EINVAL) return rc;
    if (T < 1 || T > kMaxT || Mp > kMaxRows || Mg > kMaxRows) return UAPS_ERANGE;
    return rc;
}
}  // namespace

extern "C" int uaps_detect_workspace_bytes(int B, int max_pred, int max_gt, int T, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    const int rc = check_sizes(B, max_pred, max_gt, T);
    if (rc) return rc;
    *bytes = layout(B, max_pred, max_gt).total;
    return UAPS_OK;
}

extern "C" int uaps_detect_match(const uaps_detect_call* call) {
    uaps_detect_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.pred_labels || !c.target_labels || !c.pred_count || !c.target_count || !c.pred_table || !c.target_table) return UAPS_EINVAL;
    if (!c.score || !c.rank || !c.pred_match || !c.pred_inter || !c.target_match || !c.counts || !c.workspace) return UAPS_EINVAL;
    if (c.H <= 0 || c.W <= 0 || c.max_dets < 0) return UAPS_EINVAL;
    if (c.class_agnostic != 0 && c.class_agnostic != 1) return UAPS_EINVAL;
    const int rc = check_sizes(c.B, c.max_pred, c.max_gt, c.T);
    if (rc == UAPS_EINVAL) return rc;
    if (c.num_classes < 1 || c.num_classes > UAPS_MATCH_MAX_CLASSES) return UAPS_ERANGE;
    if ((double)c.H * c.W >= kTooBig) return UAPS_ERANGE;
    if (rc) return rc;
    for (int t = 0; t < c.T; ++t)
        if (c.t1000[t] < 100 || c.t1000[t] > 1000 || (t > 0 && c.t1000[t] <= c.t1000[t - 1])) return UAPS_ERANGE;
    const Layout l = layout(c.B, c.max_pred, c.max_gt);
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, l.total)) return UAPS_EINVAL;

    DetArgs d;
    memset(&d, 0, sizeof d);
    MatchArgs& a = d.m;
    a.B = c.B; a.Mp = c.max_pred; a.Mg = c.max_gt; a.C = c.num_classes; a.agnostic = c.class_agnostic;
    a.HW = (long)c.H * c.W; a.N = (long)c.B * a.HW; a.thr = 0.0;
    a.lp = c.pred_labels; a.lg = c.target_labels; a.cnt_p = c.pred_count; a.cnt_g = c.target_count;
    a.tab_p = (const long long*)c.pred_table; a.tab_g = (const long long*)c.target_table;
    char* ws = static_cast<char*>(c.workspace);
    a.inter = reinterpret_cast<int*>(ws + l.inter);
    a.out_p = nullptr; a.out_g = nullptr; a.counts = nullptr;                  // (the sweep's counts have one writer each: nothing to zero)
    d.T = c.T; d.max_dets = c.max_dets;
    for (int t = 0; t < kMaxT; ++t) d.t1000[t] = t < c.T ? c.t1000[t] : 0;
    d.scores = c.scores; d.score = c.score;
    d.rank = (long long*)c.rank; d.pred_match = (long long*)c.pred_match; d.pred_inter = (long long*)c.pred_inter;
    d.target_match = (long long*)c.target_match; d.counts = (long long*)c.counts;
    d.cand = reinterpret_cast<int4*>(ws + l.cand); d.ncand = reinterpret_cast<int*>(ws + l.ncand);
    d.key = reinterpret_cast<u64*>(ws + l.key); d.seq = reinterpret_cast<int2*>(ws + l.seq); d.nseq = reinterpret_cast<int*>(ws + l.nseq);
    hipStream_t st = (hipStream_t)c.stream;
    const long rows_p = (long)c.B * c.max_pred;
    uaps::account_bytes(8.0 * (double)a.N + (32.0 + 16.0 * c.T) * (double)rows_p + 8.0 * c.T * c.B * (double)c.max_gt +
                        8.0 * c.B * c.num_classes * (c.T + 2.0));

    const int rc_pairs = launch_pair_count(a, rows_p, st);
    if (rc_pairs) return rc_pairs;
    hipLaunchKernelGGL(candidates_kernel, dim3((unsigned)((rows_p + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, d);
    hipLaunchKernelGGL(order_kernel, dim3((unsigned)c.B), dim3(kOrderThreads), 0, st, d);
    hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)c.B), dim3(64), 0, st, d);
    return (int)hipGetLastError();
}
