// Defect matching against ground truth for gfx950 (include/uaps_hip.h, uaps_match_instances): two results of uaps_label_instances over
// the same images -> per-defect partner / intersection / covered / matched on both sides and tp / n_pred / n_gt per image and class.
//
// The pair matrix inter[b][p - 1][g - 1] (int32, dense, in the workspace) counts the pixels that carry prediction number p and
// ground-truth number g, both with a table row and of one class (or class_agnostic).  Four launches, every one a coherence point for the
// next; integer atomics only, nothing waits inside a launch: two runs give the same bits whatever order the adds arrive in.
//   1 zero_kernel          pair_count.hpp (shared with detect.hip): the corner of every image's matrix that is read, and `counts`
//   2 pair_count_kernel<V> pair_count.hpp: both label tensors streamed once, one atomicAdd per run of equal (p, g) inside a wave
//   3 reduce_pred_kernel   one wave per (b, p): lanes stride over g, a wave max over (inter << 32) | (0xFFFFFFFF - g) gives the largest
//                          intersection and the lowest number on ties, a wave sum gives `covered`.
//   4 reduce_target_kernel one workgroup per (b, 64 columns g): lane = column (coalesced rows), the four waves split the rows p, the same
//                          packed maximum, joined in LDS.
// Both reductions run the match test on their own partner ((double) inter > threshold * (double) union); at thresholds >= 0.5 a match
// is unique and is the component's largest intersection, so the two sides agree.  n_pred, n_gt and tp reach `counts` by 64-bit integer
// atomicAdd.
#include "pair_count.hpp"

namespace {
constexpr int kRows = 8;                  // rows a lane of reduce_target_kernel reads before it compares
constexpr int kCols = 4;                  // UAPS_MATCH_COLUMNS

__device__ __forceinline__ unsigned long long pack(int inter, int number) {
    return ((unsigned long long)(unsigned)inter << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)number);
}
__device__ __forceinline__ int packed_number(unsigned long long v) { return v ? (int)(0xFFFFFFFFu - (unsigned)(v & 0xFFFFFFFFull)) : 0; }

__device__ __forceinline__ bool is_match(double thr, long long inter, long long area_a, long long area_b) {
    return (double)inter > thr * (double)(area_a + area_b - inter);
}

__global__ __launch_bounds__(kThreads) void reduce_pred_kernel(MatchArgs a) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= (long)a.B * a.Mp) return;               // (wave-uniform)
    const int b = (int)(r / a.Mp), p = (int)(r - (long)b * a.Mp);
    long long* out = a.out_p + r * kCols;
    if (p >= rows_of(a.cnt_p, b, a.Mp)) {
        if (lane < kCols) out[lane] = 0;
        return;
    }
    const int ng = rows_of(a.cnt_g, b, a.Mg);
    const int* row = a.inter + r * a.Mg;
    unsigned long long best = 0ull;
    long long cov = 0;
    for (int g = lane; g < ng; g += 64) {
        const int v = row[g];
        if (v > 0) {
            const unsigned long long k = pack(v, g + 1);
            best = k > best ? k : best;
            cov += v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(best, o, 64);
        best = t > best ? t : best;
        cov += __shfl_xor(cov, o, 64);
    }
    if (lane != 0) return;
    const long long* mine = a.tab_p + r * 9;
    const int partner = packed_number(best);
    const long long inter = (long long)(best >> 32);
    const bool m = partner > 0 && is_match(a.thr, inter, mine[1], a.tab_g[((long)b * a.Mg + partner - 1) * 9 + 1]);
    out[0] = partner; out[1] = inter; out[2] = cov; out[3] = m ? 1 : 0;
    const long long cls = mine[0];
    if (cls >= 0 && cls < a.C) atomicAdd(a.counts + ((long)b * a.C + cls) * 3 + 1, 1ull);
}

__global__ __launch_bounds__(kThreads) void reduce_target_kernel(MatchArgs a) {
    __shared__ unsigned long long s_best[kWaves][64];
    __shared__ long long s_cov[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = (a.Mg + 63) / 64;
    const int b = blockIdx.x / groups, g = (blockIdx.x - b * groups) * 64 + lane;
    const int np = rows_of(a.cnt_p, b, a.Mp), ng = rows_of(a.cnt_g, b, a.Mg);
    unsigned long long best = 0ull;
    long long cov = 0;
    if (g < ng) {
        const int* col = a.inter + (long)b * a.Mp * a.Mg + g;
        for (int p0 = wave; p0 < np; p0 += kWaves * kRows) {          // kRows independent reads in flight per lane
            int v[kRows];
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const int p = p0 + k * kWaves;
                v[k] = p < np ? col[(long)p * a.Mg] : 0;
            }
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                if (v[k] > 0) {
                    const unsigned long long w = pack(v[k], p0 + k * kWaves + 1);
                    best = w > best ? w : best;
                    cov += v[k];
                }
            }
        }
    }
    s_best[wave][lane] = best;
    s_cov[wave][lane] = cov;
    __syncthreads();
    if (wave != 0 || g >= a.Mg) return;
    long long* out = a.out_g + ((long)b * a.Mg + g) * kCols;
    if (g >= ng) {
        out[0] = 0; out[1] = 0; out[2] = 0; out[3] = 0;
        return;
    }
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        best = s_best[w][lane] > best ? s_best[w][lane] : best;
        cov += s_cov[w][lane];
    }
    const long long* mine = a.tab_g + ((long)b * a.Mg + g) * 9;
    const int partner = packed_number(best);
    const long long inter = (long long)(best >> 32);
    const bool m = partner > 0 && is_match(a.thr, inter, a.tab_p[((long)b * a.Mp + partner - 1) * 9 + 1], mine[1]);
    out[0] = partner; out[1] = inter; out[2] = cov; out[3] = m ? 1 : 0;
    const long long cls = mine[0];
    if (cls >= 0 && cls < a.C) {
        unsigned long long* row = a.counts + ((long)b * a.C + cls) * 3;
        atomicAdd(row + 2, 1ull);
        if (m) atomicAdd(row, 1ull);
    }
}
}  // namespace

extern "C" int uaps_match_workspace_bytes(int B, int max_pred, int max_gt, size_t* bytes) {
    if (!bytes) return UAPS_EINVAL;
    const int rc = check_matrix(B, max_pred, max_gt);
    if (rc) return rc;
    *bytes = align256(4 * (size_t)B * max_pred * max_gt);
    return UAPS_OK;
}

extern "C" int uaps_match_instances(const uaps_match_call* call) {
    uaps_match_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.pred_labels || !c.target_labels || !c.pred_count || !c.target_count || !c.pred_table || !c.target_table) return UAPS_EINVAL;
    if (!c.pred_out || !c.target_out || !c.counts || !c.workspace) return UAPS_EINVAL;
    if (c.H <= 0 || c.W <= 0) return UAPS_EINVAL;
    if (c.class_agnostic != 0 && c.class_agnostic != 1) return UAPS_EINVAL;
    const int rc = check_matrix(c.B, c.max_pred, c.max_gt);
    if (rc == UAPS_EINVAL) return rc;
    if (c.num_classes < 1 || c.num_classes > UAPS_MATCH_MAX_CLASSES) return UAPS_ERANGE;
    if ((double)c.H * c.W >= kTooBig) return UAPS_ERANGE;
    if (!(c.iou_threshold >= 0.5 && c.iou_threshold < 1.0)) return UAPS_ERANGE;
    if (rc) return rc;
    const size_t need = align256(4 * (size_t)c.B * c.max_pred * c.max_gt);
    if (!uaps::workspace_ok(c.workspace, c.workspace_bytes, need)) return UAPS_EINVAL;

    MatchArgs a;
    a.B = c.B; a.Mp = c.max_pred; a.Mg = c.max_gt; a.C = c.num_classes; a.agnostic = c.class_agnostic;
    a.HW = (long)c.H * c.W; a.N = (long)c.B * a.HW; a.thr = c.iou_threshold;
    a.lp = c.pred_labels; a.lg = c.target_labels; a.cnt_p = c.pred_count; a.cnt_g = c.target_count;
    a.tab_p = (const long long*)c.pred_table; a.tab_g = (const long long*)c.target_table;
    a.inter = static_cast<int*>(c.workspace);
    a.out_p = (long long*)c.pred_out; a.out_g = (long long*)c.target_out; a.counts = (unsigned long long*)c.counts;
    hipStream_t st = (hipStream_t)c.stream;
    uaps::account_bytes(8.0 * (double)a.N + 32.0 * c.B * ((double)c.max_pred + c.max_gt) + 24.0 * c.B * c.num_classes);

    const long rows_p = (long)c.B * c.max_pred;
    const long zero_waves = rows_p > (long)c.B * c.num_classes ? rows_p : (long)c.B * c.num_classes;      // >= B C 3 / kThreads blocks too
    const int rc_pairs = launch_pair_count(a, zero_waves, st);
    if (rc_pairs) return rc_pairs;
    hipLaunchKernelGGL(reduce_pred_kernel, dim3((unsigned)((rows_p + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, a);
    const long tgt_blocks = (long)c.B * ((c.max_gt + 63) / 64);
    hipLaunchKernelGGL(reduce_target_kernel, dim3((unsigned)tgt_blocks), dim3(kThreads), 0, st, a);
    return (int)hipGetLastError();
}
