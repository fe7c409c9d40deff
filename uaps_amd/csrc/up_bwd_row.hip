// The input gradient of the first convolution of up4 (3x3, 16 + 16 -> 16 channels on 256-pixel-wide maps, the second 16 input
// channels up-sampled x2 from the low-resolution tensor: UAPS_unet.py:74-75, 83-85) with the bilinear fold of its up-sampled half,
// ONE pass (include/uaps_hip.h: uaps_up_bwd_fused).
//
// Until now two HBM-bound launches ran back to back here: conv_hr16x2_kernel read dy and wrote d(skip) and d(up), both [B, 16, H, 256],
// and up_cat_bwd_low_kernel<32> read d(up) straight back to reduce it to d(low) [B, 16, H / 2, 128].  d(up) is the gradient of a tensor
// the forward never materialises (the kernels up-sample `low` while they stage it); here it never reaches memory either: dy in (1.25
// tensors with the halo rows), d(skip) and d(low) out -- 2.5 tensors of 16 channels where 4.4 moved.
//
// One workgroup of 512 threads per CU owns runs of 16 full-width rows of one image and walks down rows r0 - 1 .. r0 + 16 of a run one
// row per step; per step it fetches ONE new row of dy, two rows ahead of the row it works on, into a ring of three row slots laid out
// as conv_hr16_body's image.  The roles are split by wave (waves w and w + 4 share a SIMD):
//   * waves 0-3 stage dy (4 channels each, two fp16 pieces) and form the d(skip) half of row t (output channels 0-15) -- four 16-pixel
//     tiles per wave.  The row is handed through LDS from the matrix layout (channel = lane % 16) to the staging layout (a wave = 4
//     channels, a lane = 4 consecutive pixels) and goes to memory as whole 1-KiB rows.  The halo rows r0 - 1 and r0 + 16 are not theirs.
//   * waves 4-7 form the d(up) half of row t (output channels 16-31), the halo rows included where they lie inside the image, hand it
//     through LDS in the same way and fold it: along x in registers (one value from either neighbouring lane: the whole-wave shifts
//     of up2_staging.hpp), then along y into the two low rows that are live -- a low row is stored when its last source row has passed.
// The convolution is conv_hr16_body<2, false, 2>'s arithmetic: the same input scale from the dy bound, the same fp16 pieces and k order
// (tap, channel group), the same three-product order and output scaling, the same non-finite report.  d(skip) is that kernel's, bit
// for bit.  Ring staging, weight fragments, the row of tiles and the run walk are pieces E, F, G and I of row_pieces.hpp, shared with
// mid_bwd_row.hip; this file is the two role bodies around them, the bilinear fold and its host-side support check.
//
// Why the four-tap fold equals the seven-tap one.  Low-resolution index i draws on the output indices o whose source position
// mul_rn(r, o) lies in (i - 1, i + 1): for the x2 align_corners map these are o = 2 i - 1 .. 2 i + 2 (the entry point evaluates the
// float32 index rule on the host for the given size and refuses any size where a fifth index carries weight).  up_cat_bwd_low_kernel
// sums seven candidates 2 i - 3 .. 2 i + 3, each product rounded on its own and added left to right from a zero; the three candidates
// outside the support carry weight exactly 0 and add +-0.  Leaving them out changes nothing but, possibly, the sign of a zero result
// (for finite gradients; a non-finite one raises the error word here as there).  Same association: first along x, then along y.
// No float atomics; two launches give the same bits.
//
// Both role bodies execute the same sequence of workgroup barriers: one behind a run's first three rows, two per row (matrix work
// done; staged row in place).
//
// LDS: dy ring 50688 B + two exchange rows 33280 B = 83968 B: one workgroup per CU.
#include "../../include/uaps_hip.h"
#include "conv_kernels.hpp"
#include "conv_split.hpp"
#include "hints.hpp"
#include "row_pieces.hpp"
#include "up2_staging.hpp"

extern "C" int uaps_conv_get_mode(void);
extern "C" unsigned uaps_conv_get_tuning(void);

namespace uaps {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct UpBwdArgs {
    const float* dy;        // [B, 16, H, 256]: the gradient of the convolution's raw output
    const float* wp;        // fp16 pieces of the packed input-gradient weights [piece][tap][CGP][32] 16-byte units
    const float* wscale;    // {s, 1 / s, max|w|}
    int CGP;
    float* dskip;           // [B, 16, H, 256]
    float* dlow;            // [B, 16, H / 2, 128]
    const float* dy_bound; float dy_mul;
    float rh, rw;           // (h - 1) / (H - 1), (w - 1) / (W - 1): uaps_up_cat_bwd's
    unsigned* err;
    int B, H, nsplit;
};

// resample.hip's tap_weight: the weight of output index o in the gradient of input index i
__device__ __forceinline__ float up_fold_weight(float r, int o, int n_out, int n_in, int i) {
    if (o < 0 || o >= n_out) return 0.f;
    const float sx = mul_rn(r, (float)o);
    const int i0 = (int)sx, i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    const float l1 = sx - (float)i0, l0 = 1.f - l1;
    return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

__global__ __launch_bounds__(512, 2) void up_bwd_row_kernel(UpBwdArgs a) {
    using G = RowGeom<16>;
    constexpr int WIDTH = G::WIDTH, ROWS = G::ROWS, NTHR = 512, NCH = 4, MW = G::MW, CoutP = 32, GS = G::GS;

    __shared__ __attribute__((aligned(16))) u32x4 sIn[2 * G::PIECE];       // [piece][channel group][slot][column]
    __shared__ __attribute__((aligned(16))) float sG[2][16 * GS];          // [half][channel][column]

    const f32x2 sc = h16_scale(__builtin_fmaxf(bound_of(a.dy_bound, a.dy_mul), 0.f));
    const float in_scale = sc.x, out_scale_a = sc.y, out_scale_w = a.wscale[1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const bool is_up = wave_u >= 4;                       // which 16 output channels this wave forms
    const int half = wave_u >> 2, wq = wave_u & 3;
    const int W = WIDTH, HW = a.H * W, h = a.H / 2, w = WIDTH / 2;
    const uint32_t HW4 = (uint32_t)HW * 4u, hw4 = (uint32_t)(h * w) * 4u;

    RowRuns rr;
    if (!row_runs<G>(a.B, a.H, a.nsplit, rr)) return;

    // the margins of every row slot (image columns -4 .. -1 and 256 .. 259) are zero for the kernel's life
    zero_ring_margins<G, NTHR>(sIn, tid);

    // the weight fragments of this wave's output tile (channels half * 16 .. half * 16 + 15 of the 32 packed ones), once
    GradFrags<G> wf;
    load_grad_frags<G, CoutP>(wf, a.wp, a.CGP, half * 16 + j, j, kq, wq * MW);

    // ---- staging (waves 0-3): dy channels dc0 .. dc0 + 3 = half ch of channel group cg; lane = pixels 4 lane .. 4 lane + 3 ----
    const int dc0 = wq * NCH, cg = wq >> 1, ch = wq & 1;
    f32x4 rd[NCH];
    auto load_d = [&](int b, int gy, f32x4 (&dd)[NCH]) { load_rows4<G>(a.dy, b, gy, a.H, dc0, lane, dd); };
    auto store_d = [&](f32x4 (&dd)[NCH], int slot) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) asm volatile("" : "+v"(dd[i]));
        store_ring_rows<G>(sIn, dd, in_scale, cg, ch, lane, slot);
    };

    // ---- the fold (waves 4-7): this lane's low columns 2 lane and 2 lane + 1 draw on columns 4 lane - 1 .. 4 lane + 2 and
    // 4 lane + 1 .. 4 lane + 4 of the row (the neighbours' values come by whole-wave shifts; outside the row they are zero) ----
    float wxa[4], wxb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wxa[k] = up_fold_weight(a.rw, 4 * lane - 1 + k, W, w, 2 * lane);
        wxb[k] = up_fold_weight(a.rw, 4 * lane + 1 + k, W, w, 2 * lane + 1);
    }
    float accp[NCH][2], accq[NCH][2];                     // the two live low rows: the older (P) and the newer (Q)
#pragma unroll
    for (int i = 0; i < NCH; ++i) { accp[i][0] = accp[i][1] = 0.f; accq[i][0] = accq[i][1] = 0.f; }

    for (int run = rr.begin; run < rr.end; ++run) {
        const int b = run / rr.rpi, r0 = (run % rr.rpi) * ROWS;
        // dy rows r0 - 2, r0 - 1, r0 into slots 0, 1, 2: all fetches in flight together
        if (!is_up) {
            f32x4 da[NCH], db[NCH];
            load_d(b, r0 - 2, da);
            load_d(b, r0 - 1, db);
            load_d(b, r0, rd);
            __builtin_amdgcn_sched_barrier(0);
            store_d(da, 0);
            store_d(db, 1);
            store_d(rd, 2);
        }
        __syncthreads();
        int s0 = 0;                                       // slot of row t - 1; rows t, t + 1 follow cyclically
        const __amdgpu_buffer_rsrc_t rs_g = make_rsrc(a.dskip + (size_t)b * 16 * HW, 16u * HW4);
        const __amdgpu_buffer_rsrc_t rs_l = make_rsrc(a.dlow + (size_t)b * 16 * h * w, 16u * hw4);
#pragma unroll 1
        for (int t = r0 - 1; t <= r0 + ROWS; ++t) {
            const bool more = t < r0 + ROWS;              // step t + 1 reads row t + 2
            if (!is_up && more) load_d(b, t + 2, rd);
            int s1, s2;
            ring_slots<G>(s0, s1, s2);
            const bool own = t >= r0 && t < r0 + ROWS;
            // d(skip) exists on the run's own rows; d(up) also on the halo rows inside the image (wave-uniform)
            const bool work = is_up ? (unsigned)t < (unsigned)a.H : own;

            // ---- row t of this wave's output tile, four 16-pixel tiles: conv_hr16_body's k order and products ----
            f32x4 gacc[MW];
#pragma unroll
            for (int m = 0; m < MW; ++m) gacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (work) grad_row_tiles<G>(sIn, wf, s0, s1, s2, gacc);
            put_grad_row<G>(sG[half], gacc, out_scale_a, out_scale_w, j, kq, wq * MW, a.err);      // (a row that does not exist: zeros)
            __syncthreads();                              // every wave is done with row t - 1 of the ring; row t of both halves is complete

            if (!is_up) {
                // ---- d(skip) row t out as whole 1-KiB rows ----
                if (own) {
#pragma unroll
                    for (int i = 0; i < NCH; ++i) take_row_out<G>(sG[0], rs_g, dc0 + i, t, HW, lane);
                }
                if (more) store_d(rd, s0);
            } else {
                // ---- d(up) row t folds into the low rows (t - 1) / 2 and (t + 1) / 2 (t odd) or t / 2 - 1 and t / 2 (t even): every
                // product rounded on its own, the sums in increasing source index ----
                const bool odd = (t & 1) != 0;
                const int ip = odd ? (t - 1) / 2 : t / 2 - 1, iq = ip + 1;
                const float wyp = up_fold_weight(a.rh, t, a.H, h, ip), wyq = up_fold_weight(a.rh, t, a.H, h, iq);
                const bool out = !odd && t > r0;          // low row t / 2 - 1 of this run has seen its last source row
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    const f32x4 gv = *reinterpret_cast<const f32x4*>(&sG[1][(dc0 + i) * GS + lane * 4]);
                    const float prev = up2_lane_prev(gv[3]), next = up2_lane_next(gv[0]);
                    float ta = mul_rn(wxa[0], prev);
                    ta = add_rn(ta, mul_rn(wxa[1], gv[0])); ta = add_rn(ta, mul_rn(wxa[2], gv[1])); ta = add_rn(ta, mul_rn(wxa[3], gv[2]));
                    float tb = mul_rn(wxb[0], gv[1]);
                    tb = add_rn(tb, mul_rn(wxb[1], gv[2])); tb = add_rn(tb, mul_rn(wxb[2], gv[3])); tb = add_rn(tb, mul_rn(wxb[3], next));
                    accp[i][0] = add_rn(accp[i][0], mul_rn(wyp, ta)); accp[i][1] = add_rn(accp[i][1], mul_rn(wyp, tb));
                    if (odd) { accq[i][0] = mul_rn(wyq, ta); accq[i][1] = mul_rn(wyq, tb); }
                    else { accq[i][0] = add_rn(accq[i][0], mul_rn(wyq, ta)); accq[i][1] = add_rn(accq[i][1], mul_rn(wyq, tb)); }
                    if (!odd) {
                        const f32x2 lo = f32x2{accp[i][0], accp[i][1]};
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, lo), rs_l,
                                                              (int)(out ? (uint32_t)((dc0 + i) * h * w + ip * w + lane * 2) * 4u : kOob), 0, 0);
                        accp[i][0] = accq[i][0]; accp[i][1] = accq[i][1];
                    }
                }
            }
            s0 = s1;
            __syncthreads();
        }
    }
}

}  // namespace uaps

namespace {
// The float32 index rule of the x2 align_corners map for n_in -> 2 n_in (resample.hip: tap_weight): the smallest and largest o - 2 i
// over all (output index o, input index i) with a non-zero weight
void fold_support(int n_in, int* lo, int* hi) {
    const int n_out = 2 * n_in;
    const float r = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
    int mn = n_out, mx = -n_out;
    for (int o = 0; o < n_out; ++o) {
        volatile float sx = r * (float)o;                 // (volatile: the product rounded to float32 before it is used)
        const float s = sx;
        const int i0 = (int)s, i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
        volatile float l1v = s - (float)i0;
        const float l1 = l1v;
        volatile float l0v = 1.f - l1;
        const float l0 = l0v;
        const int is[2] = {i0, i1};
        const float ws[2] = {i0 == i1 ? l0 + l1 : l0, i0 == i1 ? 0.f : l1};
        for (int k = 0; k < 2; ++k) {
            if (ws[k] == 0.f) continue;
            const int d = o - 2 * is[k];
            if (d < mn) mn = d;
            if (d > mx) mx = d;
        }
    }
    *lo = mn; *hi = mx;
}
}  // namespace

extern "C" int uaps_up_fold_support(int n_in, int* min_offset, int* max_offset) {
    if (n_in <= 0 || n_in > (1 << 20) || !min_offset || !max_offset) return UAPS_EINVAL;
    fold_support(n_in, min_offset, max_offset);
    return UAPS_OK;
}

extern "C" int uaps_up_bwd_fused_form(int H, int W) {
    if (H <= 0 || W <= 0) return UAPS_EINVAL;
    if (W != 256 || H % 16 || H > 65536) return UAPS_ENOFORM;
    int lo = 0, hi = 0;
    fold_support(H / 2, &lo, &hi);
    if (lo < -1 || hi > 2) return UAPS_ENOFORM;
    fold_support(W / 2, &lo, &hi);
    if (lo < -1 || hi > 2) return UAPS_ENOFORM;
    return UAPS_OK;
}

extern "C" int uaps_up_bwd_fused_grid(int B, int H) {
    if (B <= 0 || H <= 0 || H % 16) return UAPS_EINVAL;
    const long nruns = (long)B * (H / 16);
    return (int)(nruns < 256 ? nruns : 256);              // one workgroup per CU
}

extern "C" int uaps_up_bwd_fused(const float* dy, const float* wb, const float* dy_bound, float dy_mul, float* dskip, int C1, float* dlow,
                                 int C2, int B, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream) {
    if (!dy || !wb || !dskip || !dlow) return UAPS_EINVAL;
    if (B <= 0 || C1 <= 0 || C2 <= 0 || Cout <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    // the one form: 3x3, 16 -> 16 + 16 channels written as two tensors, full 256-pixel rows in runs of 16, fp16-split arithmetic with
    // a bounded dy -- where uaps_conv_bwd_data_cat runs conv_hr16x2_kernel -- and a size whose fold has the four-tap support
    if (ks != 3 || Cout != 16 || C1 != 16 || C2 != 16 || W != 256 || H % 16 || H > 65536 || (cfg & ~UAPS_CONV_BOUNDED)) return UAPS_ENOFORM;
    if ((long)B * (H / 16) > 0x7fffffffL) return UAPS_ENOFORM;
    if (uaps_conv_get_mode() != 2 || !dy_bound) return UAPS_ENOFORM;
    if (uaps_conv_get_tuning() & (UAPS_TUNE_NO_SPLIT_FWD | UAPS_TUNE_NO_HP16 | UAPS_TUNE_NO_ROW16)) return UAPS_ENOFORM;
    if (((uintptr_t)dy | (uintptr_t)wb | (uintptr_t)dskip | (uintptr_t)dlow) % 16) return UAPS_ENOFORM;
    const int rc = uaps_up_bwd_fused_form(H, W);
    if (rc) return rc;
    // dy once, d(skip) and d(low) once
    uaps::account_bytes(4.0 * B * H * W * (1.0 * Cout + 1.0 * C1 + 0.25 * C2));
    uaps::UpBwdArgs a{};
    a.dy = dy;
    // the packed input-gradient weights (uaps_conv_pack_weights) as launch_fwd reads them for Cin = Cout, Cout = C1 + C2
    const uaps::H16BwdWeights w16 = uaps::h16_bwd_weights(wb, C1 + C2, Cout);
    a.wp = w16.wp; a.wscale = w16.wscale; a.CGP = w16.CGP;
    a.dskip = dskip; a.dlow = dlow;
    a.dy_bound = dy_bound; a.dy_mul = dy_mul;
    a.rh = (float)(H / 2 - 1) / (float)(H - 1); a.rw = (float)(W / 2 - 1) / (float)(W - 1);      // as uaps_up_cat_bwd
    a.err = uaps::error_word();
    a.B = B; a.H = H;
    a.nsplit = uaps_up_bwd_fused_grid(B, H);
    UAPS_LAUNCH_MAIN(uaps::up_bwd_row_kernel, dim3(uaps::row_grid(a.nsplit)), dim3(512), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
