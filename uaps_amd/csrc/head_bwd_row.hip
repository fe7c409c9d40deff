// The backward of a decoder's class convolution (out_conv: 3x3, 16 -> <= 4 channels, UAPS_unet.py:138) on 256-pixel-wide maps and the
// BatchNorm-backward sums of the layer in front of it, ONE pass (include/uaps_hip.h: uaps_head_bwd_fused).
//
// Until now three HBM-bound launches ran back to back here and read the same two tensors: the input gradient g = W^T (*) d logits
// (conv_fwd_kernel<3, 8, 32, 16, 4, 4, 1>: reads d logits, writes g), the weight gradient (conv_hrwrw_bn_kernel<1>: reads d logits and
// the raw output y of the convolution in front) and the sums pass of that layer's BatchNorm backward (bn_bwd_sums_max_kernel: reads g
// and y) -- 4.6 tensors of 16 channels moved where 2.25 are needed: d logits (a quarter) and y in, g out.
//
// The kernel is conv_hrwrw_body<1, XF = true> (conv_split_wrw_row.hpp) with two more consumers of its staged rows.  This file is its
// body: which piece of row_pieces.hpp (A - I there) runs when and between which workgroup barriers, plus what has no second user --
// the fp32 ring of d logits and the fp32 input-gradient block.  A workgroup owns runs of 16 rows of one image at full width and walks
// down them one row per step; per step it fetches ONE new row of y (16 channels, piece D) and ONE of d logits (4 channels), two rows
// ahead of the row it works on, and for row t
//   * contracts d logits row t with the activated rows t - 1, t, t + 1 of x = leaky_relu(fma(y, scale, shift)) into the nine tap
//     accumulators of dW (and the bias gradient): pieces A, B and C, which conv_hrwrw_body runs too -- its arithmetic, order and
//     slabs.  The fp16 pieces of d logits are split from the fp32 ring when the fragment is read (<= 4 channels: no second staged
//     image of it);
//   * forms g row t from the fp32 ring of d logits rows t - 1, t, t + 1 with v_mfma_f32_16x16x4_f32, one instruction per tap in
//     tap order from the fp32 GEMM layout at the front of the packed input-gradient weights: conv_fwd_body's k order, so g is
//     bit-identical to that kernel's;
//   * hands g row t through LDS from the matrix layout (channel = lane % 16) to the staging layout (a wave = 4 channels, a lane = 4
//     consecutive pixels), where the raw y row t still sits in the registers it was fetched into two steps earlier: g goes to
//     memory as whole 1-KiB rows, and bn_bwd_sums_max_kernel's per-element arithmetic runs on (g, y) in registers (piece H).
// One float2 (sum d, sum d x_hat) per (channel, image, run) goes to `partials`, summed in the order of bn_bwd_sums_max_kernel's block for
// the same 4096 floats (a run IS that kernel's chunk), so the BatchNorm coefficients are bit-identical too; the two maxima go to
// `bs_max` (uaps_bn_act_bwd_finalize's inputs).  No float atomics; two launches give the same bits.
//
// LDS: activated rows 52224 B + d logits ring 12672 B + g exchange 16640 B = 81536 B: two workgroups per CU.
#include "../../include/uaps_hip.h"
#include "conv_kernels.hpp"
#include "conv_split.hpp"
#include "hints.hpp"
#include "row_pieces.hpp"

extern "C" int uaps_conv_get_mode(void);
extern "C" unsigned uaps_conv_get_tuning(void);

namespace uaps {

struct HeadBwdArgs {
    const float* dlog;      // d logits [B, Cout, H, 256]
    const float* y;         // raw output of the convolution in front [B, 16, H, 256]
    const float* wp;        // fp32 GEMM layout of the input-gradient weights [9][4][16] (front of the packed buffer)
    float* g;               // d(activation) [B, 16, H, 256]
    const float2* xf;       // [groups][16] (scale, shift)
    float slope;            // LeakyReLU slope (0 .. 1)
    int Bg;                 // images per statistics group
    float* slab; float* bslab; int nsplit, CoutS;
    const float* dy_bound; const float* in_bound;
    float dy_mul, in_mul;
    const float* bs_mean; const float* bs_invstd; const float* bs_gamma; const float* bs_beta;
    float2* partials;       // [16][B][H / 16]
    float* bs_max;          // two bounds: max|d|, max|x_hat|
    unsigned* err;
    int B, Cout, H;
};

__global__ __launch_bounds__(256, 2) void head_bwd_row_kernel(HeadBwdArgs a) {
    using G = RowGeom<16>;
    constexpr int WIDTH = G::WIDTH, NSLOT = G::NSLOT, ROWS = G::ROWS, CI = G::CI, NTHR = 256, NXL = G::NXL, GS = G::GS;
    constexpr int DW = WIDTH + 8;                         // floats of a d-logits ring row: 4 of margin either side (columns -1 and 256 are zero)
    constexpr int RED_FLOATS = 2 * 10 * 256;
    static_assert(RED_FLOATS / 4 <= G::X_UNITS, "the reduction scratch fits the input image");

    __shared__ __attribute__((aligned(16))) u32x4 sX[G::X_UNITS];          // [piece][ci][slot][group]
    __shared__ __attribute__((aligned(16))) float sDf[4 * NSLOT * DW];     // [co][slot][column]
    __shared__ __attribute__((aligned(16))) float sG[16 * GS];             // [ci][column]

    const f32x2 sd = h16_scale(bound_of(a.dy_bound, a.dy_mul));
    const f32x2 sx = h16_scale(bound_of(a.in_bound, a.in_mul));
    const float sc_d = sd.x, inv_d = sd.y, sc_x = sx.x, inv_x = sx.y;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int sp = wave_u;                                // segment pair (K split) of this wave's weight-gradient work
    const int W = WIDTH, HW = a.H * W;
    const uint32_t HW4 = (uint32_t)HW * 4u;

    RowRuns rr;
    if (!row_runs<G>(a.B, a.H, a.nsplit, rr)) return;
    const bool want_bias = a.bslab != nullptr;

    // zero halo groups of the activated rows and the margins of the d-logits ring, for the kernel's life
    zero_x_halo<G, NTHR>(sX, tid);
    for (int e = tid; e < 4 * NSLOT * 8; e += NTHR) sDf[(e / 8) * DW + (e % 8 < 4 ? e % 8 : WIDTH + e % 8)] = 0.f;

    // input-gradient weights: lane (n = j, k = kq) of tap t holds wp[t][kq][j]
    float bw[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) bw[t] = a.wp[(t * 4 + kq) * 16 + j];

    // ---- staging: lane = pixels 4 lane .. 4 lane + 3 of y channels 4 wave .. 4 wave + 3 and of d-logits channel `wave` ----
    f32x4 rx[NXL], xa[NXL], xb[NXL], rd;
    BnRowSums<G> bn;
    bool x_in = false;
    const int xc0 = wave_u * NXL;
    auto load_d = [&](int b, int gy, f32x4& dst) {        // rows outside the image and absent channels read zeros
        const bool ok = (unsigned)gy < (unsigned)a.H && wave_u < a.Cout;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.dlog + (size_t)b * a.Cout * HW, (uint32_t)a.Cout * HW4);
        dst = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(ok ? (uint32_t)(wave_u * HW + gy * W + lane * 4) * 4u : kOob), 0, 0));
    };
    auto store_x = [&](f32x4 (&src)[NXL], bool ok, int slot) { store_act_rows<G>(sX, src, bn.cf, ok, a.slope, sc_x, xc0, lane, slot); };
    auto store_d = [&](f32x4& src, int slot) {
        asm volatile("" : "+v"(src));
        *reinterpret_cast<f32x4*>(&sDf[(wave_u * NSLOT + slot) * DW + 4 + lane * 4]) = src;
    };

    f32x4 acc[9];
    f32x4 accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bs_md = 0.f, bs_mx = 0.f;

    for (int run = rr.begin; run < rr.end; ++run) {
        const int b = run / rr.rpi, r0 = (run % rr.rpi) * ROWS;
        bn_run_begin(bn, a.xf, a.bs_mean, a.bs_invstd, a.bs_gamma, a.bs_beta, b / a.Bg, xc0);
        // rows r0 - 1, r0, r0 + 1 of both operands into slots 0, 1, 2: all fetches in flight together
        {
            f32x4 ra[NXL], da, db;
            const bool oka = load_rows4<G>(a.y, b, r0 - 1, a.H, xc0, lane, ra);
            const bool okb = load_rows4<G>(a.y, b, r0, a.H, xc0, lane, xa);
            x_in = load_rows4<G>(a.y, b, r0 + 1, a.H, xc0, lane, xb);
            load_d(b, r0 - 1, da); load_d(b, r0, db); load_d(b, r0 + 1, rd);
            __builtin_amdgcn_sched_barrier(0);
            store_x(ra, oka, 0);
            store_x(xa, okb, 1);
            store_x(xb, x_in, 2);
            store_d(da, 0); store_d(db, 1); store_d(rd, 2);
        }
        __syncthreads();
        int s0 = 0;                                       // slot of row t - 1 (both rings); rows t, t + 1 follow cyclically
        const __amdgpu_buffer_rsrc_t rs_g = make_rsrc(a.g + (size_t)b * CI * HW, (uint32_t)CI * HW4);
#pragma unroll 1
        for (int t = r0; t < r0 + ROWS; ++t) {
            const bool more = t + 1 < r0 + ROWS;
            if (more) { x_in = load_rows4<G>(a.y, b, t + 2, a.H, xc0, lane, rx); load_d(b, t + 2, rd); }
            int s1, s2;
            ring_slots<G>(s0, s1, s2);
            const auto slot_of = [&](int ky) { return ky == 0 ? s0 : (ky == 1 ? s1 : s2); };

            // ---- weight gradient: d-logits row t against the activated rows t - 1, t, t + 1 (piece A) ----
#pragma unroll
            for (int sgi = 0; sgi < 2; ++sgi) {
                const int gq = (sp * 2 + sgi) * 4 + kq;   // this lane's 8-pixel group of the row
                f16x8 af[2];                              // the fp16 pieces of d logits, split from the fp32 ring as the fragment is read
                {
                    const float* dp = &sDf[((j & 3) * NSLOT + s1) * DW + 4 + 8 * gq];
                    const f32x4 u0 = *reinterpret_cast<const f32x4*>(dp), u1 = *reinterpret_cast<const f32x4*>(dp + 4);
                    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
                    conv_split2h(u0.x * sc_d, u0.y * sc_d, h0, l0);
                    conv_split2h(u0.z * sc_d, u0.w * sc_d, h1, l1);
                    conv_split2h(u1.x * sc_d, u1.y * sc_d, h2, l2);
                    conv_split2h(u1.z * sc_d, u1.w * sc_d, h3, l3);
                    const bool real = j < 4;              // output channels 4 .. 15 of the 16-row fragment do not exist
                    af[0] = __builtin_bit_cast(f16x8, real ? u32x4{h0, h1, h2, h3} : u32x4{0u, 0u, 0u, 0u});
                    af[1] = __builtin_bit_cast(f16x8, real ? u32x4{l0, l1, l2, l3} : u32x4{0u, 0u, 0u, 0u});
                }
                tap_contract<G>(sX, af, j, gq, slot_of, want_bias, acc, accb);
            }

            // ---- input gradient: g row t, this wave's four 16-pixel tiles; lane (j, kq) ends with pixels 4 kq .. 4 kq + 3 of channel j ----
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int px = (wave_u * 4 + m) * 16;
                f32x4 gacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int slot = tap / 3 == 0 ? s0 : (tap / 3 == 1 ? s1 : s2);
                    const float av = sDf[(kq * NSLOT + slot) * DW + 3 + px + j + tap % 3];
                    gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[tap], gacc, 0, 0, 0);
                }
                gacc += 0.f;                              // (the tile kernel adds its absent bias)
                *reinterpret_cast<f32x4*>(&sG[j * GS + px + kq * 4]) = gacc;
            }
            __syncthreads();                              // every wave is done with row t - 1 of both rings; g row t is complete

            // ---- g row t out, and the BatchNorm-backward sums of (g, y) row t (piece H) ----
#pragma unroll
            for (int i = 0; i < NXL; ++i) bn_row(bn, i, take_row_out<G>(sG, rs_g, xc0 + i, t, HW, lane), xa[i], a.slope, bs_md, bs_mx);
            if (more) { store_x(rx, x_in, s0); store_d(rd, s0); }
#pragma unroll
            for (int i = 0; i < NXL; ++i) { xa[i] = xb[i]; xb[i] = rx[i]; }
            s0 = s1;
            __syncthreads();
        }
        bn_run_end(bn, a.partials, a.B, b, rr.rpi, r0 / ROWS, xc0, lane);
    }

    ksplit_reduce<1>(reinterpret_cast<float*>(sX), sp, 0, lane, acc, accb);
    block_amax_to(a.bs_max, bs_md, sG);                    // (sG is dead; every thread of the workgroup gets here)
    block_amax_to(a.bs_max + UAPS_BOUND_FLOATS, bs_mx, sG + 16);
    if (sp != 0) return;
    store_slabs(a.slab, a.bslab, want_bias, rr.split, a.CoutS, CI, 0, j, kq, acc, accb, inv_d, inv_x, a.err);
}

}  // namespace uaps

extern "C" int uaps_head_bwd_fused(const float* dlogits, const float* y, const void* xf, float slope, int groups, const float* wb,
                                   const float* dy_bound, float dy_mul, const float* x_bound, float x_mul, const float* save_mean,
                                   const float* save_invstd, const float* gamma, const float* beta, int want_bias, int B, int Cin,
                                   int Cout, int H, int W, int ks, int cfg, float* g, void* partials, float* maxes, void* ws,
                                   size_t ws_bytes, uaps_stream_t stream) {
    if (!dlogits || !y || !xf || !wb || !save_mean || !save_invstd || !gamma || !beta || !g || !partials || !maxes || !ws) return UAPS_EINVAL;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || groups < 1 || B % groups || (uintptr_t)xf % 8) return UAPS_EINVAL;
    if (!(slope >= 0.f && slope <= 1.f)) return UAPS_ERANGE;      // leaky_relu is evaluated as max(z, slope * z)
    // the one form: 3x3, 16 -> <= 4 channels, full 256-pixel rows in runs of 16, fp16-split arithmetic with both operands bounded
    if (ks != 3 || Cin != 16 || Cout > 4 || W != 256 || H % 16 || H > 65536 || (cfg & ~0x3ff)) return UAPS_ENOFORM;
    if (uaps_conv_get_mode() != 2 || !dy_bound || !x_bound) return UAPS_ENOFORM;
    if (uaps_conv_get_tuning() & (UAPS_TUNE_NO_ROW_WRW | UAPS_TUNE_NO_SPLIT_WRW)) return UAPS_ENOFORM;
    if (((uintptr_t)dlogits | (uintptr_t)y | (uintptr_t)g | (uintptr_t)wb | (uintptr_t)ws) % 16) return UAPS_ENOFORM;
    uaps::HeadBwdArgs a{};
    a.CoutS = 4;                                           // the exact-N slab layout [split][tap][4][16] + [split][4]
    const int rc = uaps::row_wrw_bn_args(a, a.CoutS, B, Cin, Cout, H, W, ks, cfg, want_bias, ws, ws_bytes, dy_bound, dy_mul, x_bound, x_mul,
                                         save_mean, save_invstd, gamma, beta, partials, maxes);
    if (rc) return rc;
    // d logits and y in, g out: each once
    uaps::account_bytes(4.0 * B * H * W * ((double)Cout + 2.0 * Cin));
    a.dlog = dlogits; a.y = y; a.wp = wb; a.g = g;
    a.xf = (const float2*)xf; a.slope = slope; a.Bg = B / groups;
    a.B = B; a.Cout = Cout; a.H = H;
    UAPS_LAUNCH_MAIN(uaps::head_bwd_row_kernel, dim3(uaps::row_grid(a.nsplit)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
