// The backward of the second convolution of a decoder ConvBlock on 256-pixel-wide maps (conv2: 3x3, 16 -> 16 channels, UAPS_unet.py:38-44)
// and the BatchNorm-backward sums of the layer in front of it, ONE pass (include/uaps_hip.h: uaps_mid_bwd_fused).
//
// Until now three HBM-bound launches ran back to back here: conv2's weight gradient (conv_hrwrw_bn_dt_kernel<1>: reads d(act2), y2 and
// y1, forms the true dy2 while staging and WRITES it through), conv2's input gradient (conv_hr16_kernel<2>: reads dy2 back, writes
// d(act1)) and the sums pass of BatchNorm 1's backward (bn_bwd_sums_max_kernel: reads d(act1) back, and y1 again) -- 8.3 tensors of 16
// channels moved where 4 are needed: d(act2), y2 and y1 in, d(act1) out.  dy2 never reaches memory here.
//
// One workgroup of 512 threads per CU owns runs of 16 full-width rows of one image and walks down them one row per step; per step
// it fetches ONE new row of each input tensor, two rows ahead of the row it works on.  The roles are split by wave, so that every wave
// carries only its own accumulators and weight fragments (waves w and w + 4 share a SIMD).  This file is the two role bodies: which
// piece of row_pieces.hpp (A - I there) runs when, and between which workgroup barriers; the arithmetic is the pieces'.
//   * waves 0-3 stage dy2: a wave fetches whole 1-KiB rows of 4 channels of d(act2) and y2 (4 pixels per lane), forms dy2 with
//     store_d's expression of conv_split_wrw_row.hpp and stores its two fp16 pieces in BOTH layouts the contractions read -- the
//     pixel-grouped row [piece][co][8-pixel group] (two alternating rows) and the channel-grouped ring (piece E; three rows; rows
//     outside the image are zero).  Then they contract dy2 row t with the activated rows t - 1, t, t + 1 of x = leaky_relu(fma(y1,
//     scale, shift)) into the nine tap accumulators (and the bias gradient): pieces A, B and C, which conv_hrwrw_body<1, XF, DT> runs
//     too -- its arithmetic, order, slabs and cross-wave reduction.  The halo rows r0 - 1 and r0 + 16 of a run go to the ring only.
//   * waves 4-7 stage y1 (piece D: 4 channels each, activated and split into the x ring, the raw rows t, t + 1, t + 2 kept in
//     registers) and form d(act1) row t from the dy2 ring rows t - 1, t, t + 1 (pieces F and G: conv_hr16_body<2, false>'s input
//     scale, fp16 pieces, k order and product order, four 16-pixel tiles per wave).  The row is handed through LDS from the matrix
//     layout (channel = lane % 16) to the staging layout (a wave = 4 channels, a lane = 4 consecutive pixels), goes to memory as
//     whole 1-KiB rows, and bn_bwd_sums_max_kernel's per-element arithmetic runs on (d(act1), y1) in registers (piece H).
// One float2 (sum d, sum d x_hat) per (channel, image, run) goes to `partials` in the order of bn_bwd_sums_max_kernel's block for the
// same 4096 floats, the two maxima to `bs_max` (uaps_bn_act_bwd_finalize's inputs).  No float atomics; two launches give the same bits.
//
// Both role bodies execute the same sequence of workgroup barriers: one behind a run's first three rows, two per row (matrix work done;
// staged rows in place), four in the cross-wave reduction of the weight gradient (piece B).
//
// LDS: activated rows 52224 B + dy2 row pair 32768 B + dy2 ring 50688 B + d(act1) exchange 16640 B = 152320 B: one workgroup per CU.
#include "../../include/uaps_hip.h"
#include "conv_kernels.hpp"
#include "conv_split.hpp"
#include "hints.hpp"
#include "row_pieces.hpp"

extern "C" int uaps_conv_get_mode(void);
extern "C" unsigned uaps_conv_get_tuning(void);

namespace uaps {

struct MidBwdArgs {
    const float* dact;      // d(act2) [B, 16, H, 256]: the gradient behind conv2's BatchNorm + LeakyReLU
    const float* y2;        // raw output of conv2 [B, 16, H, 256]
    const float* coef;      // [groups2][16][8]: uaps_bn_act_bwd_prepare's table for (d(act2), y2)
    float dt_slope;
    int dt_Bg;
    const float* y1;        // raw output of conv1 [B, 16, H, 256]
    const float2* xf;       // [groups][16] (scale, shift)
    float slope;            // LeakyReLU slope behind BatchNorm 1 (0 .. 1)
    int Bg;                 // images per statistics group of BatchNorm 1
    const float* wp;        // fp16 pieces of the packed input-gradient weights [piece][tap][CGP][16] 16-byte units
    const float* wscale;    // {s, 1 / s, max|w|}
    int CGP;
    float* g;               // d(act1) [B, 16, H, 256]
    float* slab; float* bslab; int nsplit;
    const float* dy_bound; const float* in_bound;
    float dy_mul, in_mul;
    const float* bs_mean; const float* bs_invstd; const float* bs_gamma; const float* bs_beta;
    float2* partials;       // [16][B][H / 16]
    float* bs_max;          // two bounds: max|d|, max|x_hat|
    unsigned* err;
    int B, H;
};

__global__ __launch_bounds__(512, 2) void mid_bwd_row_kernel(MidBwdArgs a) {
    using G = RowGeom<16>;
    constexpr int NG = G::NG, ROWS = G::ROWS, CI = G::CI, NTHR = 512, NXL = G::NXL, MW = G::MW, D_UNITS = G::D_UNITS;
    constexpr int RED_FLOATS = 2 * 10 * 256;
    static_assert(RED_FLOATS / 4 <= G::X_UNITS, "the reduction scratch fits the input image");

    __shared__ __attribute__((aligned(16))) u32x4 sX[G::X_UNITS];          // [piece][ci][slot][group]
    __shared__ __attribute__((aligned(16))) u32x4 sD[2 * D_UNITS];         // [row parity][piece][co][group]
    __shared__ __attribute__((aligned(16))) u32x4 sIn[2 * G::PIECE];       // [piece][channel group][slot][column]
    __shared__ __attribute__((aligned(16))) float sG[16 * G::GS];          // [ci][column]

    const f32x2 sd = h16_scale(__builtin_fmaxf(bound_of(a.dy_bound, a.dy_mul), 0.f));
    const f32x2 sx = h16_scale(__builtin_fmaxf(bound_of(a.in_bound, a.in_mul), 0.f));
    const float sc_d = sd.x, inv_d = sd.y, sc_x = sx.x, inv_x = sx.y;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int HW = a.H * G::WIDTH;
    const uint32_t HW4 = (uint32_t)HW * 4u;

    RowRuns rr;
    if (!row_runs<G>(a.B, a.H, a.nsplit, rr)) return;

    // zero halo groups of the activated rows and the margins of the dy2 ring, for the kernel's life
    zero_x_halo<G, NTHR>(sX, tid);
    zero_ring_margins<G, NTHR>(sIn, tid);

    float bs_md = 0.f, bs_mx = 0.f;

    if (wave_u < 4) {
        // =========================== waves 0-3: dy2 staging and the weight gradient ===========================
        const int sp = wave_u;                            // segment pair (K split) of this wave's weight-gradient work
        const int dc0 = wave_u * 4, cg = wave_u >> 1, ch = wave_u & 1;      // staging: dy2 channels dc0 .. dc0 + 3 = half ch of channel group cg; lane = pixels 4 lane .. 4 lane + 3
        const bool want_bias = a.bslab != nullptr;
        f32x4 rd[4], ry[4];
        bool d_in = false;
        float dtc[4][6];                                  // (mean, invstd, gamma invstd, beta, mean(d), mean(d x_hat)) of this wave's dy2 channels
        auto load_d = [&](int b, int gy, f32x4 (&dd)[4], f32x4 (&yy)[4], bool& ok) {
            ok = load_rows4<G>(a.dact, b, gy, a.H, dc0, lane, dd);
            load_rows4<G>(a.y2, b, gy, a.H, dc0, lane, yy);
        };
        // dy2 = sc (d - k2 - x_hat k3), d = g or slope g by the sign of the BatchNorm output (conv_split_wrw_row.hpp: store_d); rows outside
        // the image are zero.  buf < 0: a halo row, which the weight gradient must not see
        auto store_d = [&](f32x4 (&dd)[4], f32x4 (&yy)[4], bool ok, int slot, int buf) {
            f32x4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                asm volatile("" : "+v"(dd[i]));
                asm volatile("" : "+v"(yy[i]));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float g0 = dd[i][k];
                    const float yc = yy[i][k] - dtc[i][0];
                    const float z = yc * dtc[i][2] + dtc[i][3];
                    const float d = z > 0.f ? g0 : g0 * a.dt_slope;
                    const float t = dtc[i][2] * (d - dtc[i][4] - (yc * dtc[i][1]) * dtc[i][5]);
                    v[i][k] = ok ? t : 0.f;
                }
            }
            store_ring_rows<G>(sIn, v, sc_d, cg, ch, lane, slot);
            if (buf >= 0) {                               // the row: conv_hrwrw_body's image
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    unsigned a0, a1, b0, b1;
                    conv_split2h(v[i][0] * sc_d, v[i][1] * sc_d, a0, a1);
                    conv_split2h(v[i][2] * sc_d, v[i][3] * sc_d, b0, b1);
                    const int c = dc0 + i;
                    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned*>(&sD[buf * D_UNITS + c * NG]) + lane * 2) = make_uint2(a0, b0);
                    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned*>(&sD[buf * D_UNITS + (16 + c) * NG]) + lane * 2) = make_uint2(a1, b1);
                }
            }
        };

        f32x4 acc[9];
        f32x4 accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int run = rr.begin; run < rr.end; ++run) {
            const int b = run / rr.rpi, r0 = (run % rr.rpi) * ROWS;
            const int grp2 = b / a.dt_Bg;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 6; ++k) dtc[i][k] = a.coef[((size_t)grp2 * 16 + dc0 + i) * 8 + k];
            // dy2 rows r0 - 1, r0, r0 + 1 into slots 0, 1, 2: all fetches in flight together
            {
                f32x4 da[4], ya[4], db[4], yb[4];
                bool oka, okb;
                load_d(b, r0 - 1, da, ya, oka);
                load_d(b, r0, db, yb, okb);
                load_d(b, r0 + 1, rd, ry, d_in);
                __builtin_amdgcn_sched_barrier(0);
                store_d(da, ya, oka, 0, -1);
                store_d(db, yb, okb, 1, 0);
                store_d(rd, ry, d_in, 2, 1);
            }
            __syncthreads();
            int s0 = 0, buf = 0;                          // slot of row t - 1 (both rings); parity of dy2 row t
#pragma unroll 1
            for (int t = r0; t < r0 + ROWS; ++t) {
                const bool more = t + 1 < r0 + ROWS;
                if (more) load_d(b, t + 2, rd, ry, d_in);
                int s1, s2;
                ring_slots<G>(s0, s1, s2);
                const auto slot_of = [&](int ky) { return ky == 0 ? s0 : (ky == 1 ? s1 : s2); };
                const u32x4* sDb = sD + buf * D_UNITS;
                // ---- dy2 row t against the activated rows t - 1, t, t + 1 ----
#pragma unroll
                for (int sgi = 0; sgi < 2; ++sgi) {
                    const int gq = (sp * 2 + sgi) * 4 + kq;       // this lane's 8-pixel group of the row
                    f16x8 af[2];
                    read_dy_frag<G>(sDb, j, gq, af);
                    tap_contract<G>(sX, af, j, gq, slot_of, want_bias, acc, accb);
                }
                __syncthreads();                          // every wave is done with row t - 1 of both rings and with dy2 row t
                if (more) store_d(rd, ry, d_in, s0, buf);
                s0 = s1; buf ^= 1;
                __syncthreads();
            }
        }

        ksplit_reduce<1>(reinterpret_cast<float*>(sX), sp, 0, lane, acc, accb);
        if (sp == 0) store_slabs<true>(a.slab, a.bslab, want_bias, rr.split, 16, CI, 0, j, kq, acc, accb, inv_d, inv_x, a.err);
    } else {
        // =========================== waves 4-7: y1 staging, the input gradient and the BatchNorm-backward sums ===========================
        const int wg = wave_u - 4;
        const int xc0 = wg * NXL;                         // staging: y1 channels xc0 .. xc0 + 3, lane = pixels 4 lane .. 4 lane + 3
        const float out_scale_a = inv_d, out_scale_w = a.wscale[1];      // (the input scale is sc_d: lz.bound bounds dy2 for both contractions)

        GradFrags<G> wf;
        load_grad_frags<G, 16>(wf, a.wp, a.CGP, j, j, kq, wg * MW);

        f32x4 rx[NXL], xa[NXL], xb[NXL];
        BnRowSums<G> bn;
        bool x_in = false;
        auto store_x = [&](f32x4 (&src)[NXL], bool ok, int slot) { store_act_rows<G>(sX, src, bn.cf, ok, a.slope, sc_x, xc0, lane, slot); };

        for (int run = rr.begin; run < rr.end; ++run) {
            const int b = run / rr.rpi, r0 = (run % rr.rpi) * ROWS;
            bn_run_begin(bn, a.xf, a.bs_mean, a.bs_invstd, a.bs_gamma, a.bs_beta, b / a.Bg, xc0);
            // y1 rows r0 - 1, r0, r0 + 1 into slots 0, 1, 2: all fetches in flight together
            {
                f32x4 ra[NXL];
                const bool oka = load_rows4<G>(a.y1, b, r0 - 1, a.H, xc0, lane, ra);
                const bool okb = load_rows4<G>(a.y1, b, r0, a.H, xc0, lane, xa);
                x_in = load_rows4<G>(a.y1, b, r0 + 1, a.H, xc0, lane, xb);
                __builtin_amdgcn_sched_barrier(0);
                store_x(ra, oka, 0);
                store_x(xa, okb, 1);
                store_x(xb, x_in, 2);
            }
            __syncthreads();
            int s0 = 0;                                   // slot of row t - 1 (both rings); rows t, t + 1 follow cyclically
            const __amdgpu_buffer_rsrc_t rs_g = make_rsrc(a.g + (size_t)b * CI * HW, (uint32_t)CI * HW4);
#pragma unroll 1
            for (int t = r0; t < r0 + ROWS; ++t) {
                const bool more = t + 1 < r0 + ROWS;
                if (more) x_in = load_rows4<G>(a.y1, b, t + 2, a.H, xc0, lane, rx);
                int s1, s2;
                ring_slots<G>(s0, s1, s2);

                // ---- d(act1) row t, this wave's four 16-pixel tiles ----
                f32x4 gacc[MW];
#pragma unroll
                for (int m = 0; m < MW; ++m) gacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
                grad_row_tiles<G>(sIn, wf, s0, s1, s2, gacc);
                put_grad_row<G>(sG, gacc, out_scale_a, out_scale_w, j, kq, wg * MW, a.err);
                __syncthreads();                          // every wave is done with row t - 1 of both rings; d(act1) row t is complete

                // ---- d(act1) row t out, and the BatchNorm-backward sums of (d(act1), y1) row t ----
#pragma unroll
                for (int i = 0; i < NXL; ++i) bn_row(bn, i, take_row_out<G>(sG, rs_g, xc0 + i, t, HW, lane), xa[i], a.slope, bs_md, bs_mx);
                if (more) store_x(rx, x_in, s0);
#pragma unroll
                for (int i = 0; i < NXL; ++i) { xa[i] = xb[i]; xb[i] = rx[i]; }
                s0 = s1;
                __syncthreads();
            }
            bn_run_end(bn, a.partials, a.B, b, rr.rpi, r0 / ROWS, xc0, lane);
        }
        // (the four barriers of the weight gradient's cross-wave reduction)
        __syncthreads(); __syncthreads(); __syncthreads(); __syncthreads();
    }
    block_amax_to(a.bs_max, bs_md, sG);                    // (sG is dead; every thread of the workgroup gets here)
    block_amax_to(a.bs_max + UAPS_BOUND_FLOATS, bs_mx, sG + 16);
}

}  // namespace uaps

extern "C" int uaps_mid_bwd_fused(const float* dact, const float* y2, const float* coef, float slope2, int groups2, const float* y1,
                                  const void* xf, float slope, int groups, const float* wb, const float* dy_bound, float dy_mul,
                                  const float* x_bound, float x_mul, const float* save_mean, const float* save_invstd,
                                  const float* gamma, const float* beta, int want_bias, int B, int Cin, int Cout, int H, int W, int ks,
                                  int cfg, float* g, void* partials, float* maxes, void* ws, size_t ws_bytes, uaps_stream_t stream) {
    if (!dact || !y1 || !xf || !wb || !save_mean || !save_invstd || !gamma || !beta || !g || !partials || !maxes || !ws) return UAPS_EINVAL;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || groups < 1 || B % groups || (uintptr_t)xf % 8) return UAPS_EINVAL;
    if ((y2 || coef) && (!y2 || !coef || groups2 < 1 || B % groups2)) return UAPS_EINVAL;
    if (!(slope >= 0.f && slope <= 1.f)) return UAPS_ERANGE;      // leaky_relu is evaluated as max(z, slope * z)
    // the one form: 3x3, 16 -> 16 channels, full 256-pixel rows in runs of 16, fp16-split arithmetic with both operands bounded and a
    // pending BatchNorm transform on the incoming gradient
    if (ks != 3 || Cin != 16 || Cout != 16 || W != 256 || H % 16 || H > 65536 || (cfg & ~0x3ff)) return UAPS_ENOFORM;
    if (!y2 || !coef) return UAPS_ENOFORM;
    if (uaps_conv_get_mode() != 2 || !dy_bound || !x_bound) return UAPS_ENOFORM;
    if (uaps_conv_get_tuning() & (UAPS_TUNE_NO_ROW_WRW | UAPS_TUNE_NO_SPLIT_WRW)) return UAPS_ENOFORM;
    if (((uintptr_t)dact | (uintptr_t)y2 | (uintptr_t)y1 | (uintptr_t)g | (uintptr_t)wb | (uintptr_t)ws | (uintptr_t)coef) % 16) return UAPS_ENOFORM;
    uaps::MidBwdArgs a{};
    const int rc = uaps::row_wrw_bn_args(a, 16, B, Cin, Cout, H, W, ks, cfg, want_bias, ws, ws_bytes, dy_bound, dy_mul, x_bound, x_mul,
                                         save_mean, save_invstd, gamma, beta, partials, maxes);
    if (rc) return rc;
    // d(act2), y2 and y1 in, d(act1) out: each once
    uaps::account_bytes(4.0 * B * H * W * (3.0 * Cout + 1.0 * Cin));
    a.dact = dact; a.y2 = y2; a.coef = coef; a.dt_slope = slope2; a.dt_Bg = B / groups2;
    a.y1 = y1; a.xf = (const float2*)xf; a.slope = slope; a.Bg = B / groups;
    const uaps::H16BwdWeights w16 = uaps::h16_bwd_weights(wb, Cin, Cout);
    a.wp = w16.wp; a.wscale = w16.wscale; a.CGP = w16.CGP;
    a.g = g;
    a.B = B; a.H = H;
    UAPS_LAUNCH_MAIN(uaps::mid_bwd_row_kernel, dim3(uaps::row_grid(a.nsplit)), dim3(512), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
