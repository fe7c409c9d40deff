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
// carries only its own accumulators and weight fragments (waves w and w + 4 share a SIMD):
//   * waves 0-3 stage dy2: a wave fetches whole 1-KiB rows of 4 channels of d(act2) and y2 (4 pixels per lane), forms dy2 with
//     store_d's expression of conv_split_wrw_row.hpp and stores its two fp16 pieces in BOTH layouts the contractions read -- the
//     pixel-grouped row [piece][co][8-pixel group] (two alternating rows) and the channel-grouped ring [piece][channel group][slot]
//     [column] (three rows; rows outside the image are zero).  Then they contract dy2 row t with the activated rows t - 1, t, t + 1
//     of x = leaky_relu(fma(y1, scale, shift)) into the nine tap accumulators (and the bias gradient): conv_hrwrw_body<1, XF, DT>'s
//     arithmetic, order, slabs and cross-wave reduction, bit for bit.  The halo rows r0 - 1 and r0 + 16 of a run go to the ring only.
//   * waves 4-7 stage y1 (4 channels each, activated and split into the x ring, the raw rows t, t + 1, t + 2 kept in registers) and
//     form d(act1) row t from the dy2 ring rows t - 1, t, t + 1 with conv_hr16_body<2, false>'s arithmetic: the same input scale,
//     fp16 pieces, k order (tap, channel group) and product order, four 16-pixel tiles per wave.  The row is handed through LDS from
//     the matrix layout (channel = lane % 16) to the staging layout (a wave = 4 channels, a lane = 4 consecutive pixels), goes to
//     memory as whole 1-KiB rows, and bn_bwd_sums_max_kernel's per-element arithmetic runs on (d(act1), y1) in registers.
// One float2 (sum d, sum d x_hat) per (channel, image, run) goes to `partials` in the order of bn_bwd_sums_max_kernel's block for the
// same 4096 floats, the two maxima to `bs_max` (uaps_bn_act_bwd_finalize's inputs).  No float atomics; two launches give the same bits.
//
// Both role bodies execute the same sequence of workgroup barriers: one behind a run's first three rows, two per row (matrix work done;
// staged rows in place), four in the cross-wave reduction of the weight gradient.
//
// LDS: activated rows 52224 B + dy2 row pair 32768 B + dy2 ring 50688 B + d(act1) exchange 16640 B = 152320 B: one workgroup per CU.
#include "../../include/uaps_hip.h"
#include "conv_kernels.hpp"
#include "conv_split.hpp"
#include "hints.hpp"

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
    constexpr int WIDTH = 256, NG = WIDTH / 8, XG = NG + 2, NSLOT = 3, ROWS = 16, CI = 16, NTHR = 512, NXL = 4;
    constexpr int X_UNITS = 2 * CI * NSLOT * XG;
    constexpr int D_UNITS = 2 * 16 * NG;                  // one pixel-grouped dy2 row, both pieces
    constexpr int IW = WIDTH + 8, CGU = NSLOT * IW, PIECE = 2 * CGU, XS = 3;      // the dy2 ring: conv_hr16_body's image with three row slots
    constexpr int NQ = 9 * 2, NSTEP = (NQ + 3) / 4, MW = 4;
    constexpr int GS = WIDTH + 4;                         // channel stride of the d(act1) exchange image
    constexpr int RED_FLOATS = 2 * 10 * 256;
    static_assert(RED_FLOATS / 4 <= X_UNITS, "the reduction scratch fits the input image");

    __shared__ __attribute__((aligned(16))) u32x4 sX[X_UNITS];             // [piece][ci][slot][group]
    __shared__ __attribute__((aligned(16))) u32x4 sD[2 * D_UNITS];         // [row parity][piece][co][group]
    __shared__ __attribute__((aligned(16))) u32x4 sIn[2 * PIECE];          // [piece][channel group][slot][column]
    __shared__ __attribute__((aligned(16))) float sG[16 * GS];             // [ci][column]

    const f32x2 sd = h16_scale(__builtin_fmaxf(bound_of(a.dy_bound, a.dy_mul), 0.f));
    const f32x2 sx = h16_scale(__builtin_fmaxf(bound_of(a.in_bound, a.in_mul), 0.f));
    const float sc_d = sd.x, inv_d = sd.y, sc_x = sx.x, inv_x = sx.y;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int W = WIDTH, HW = a.H * W;
    const uint32_t HW4 = (uint32_t)HW * 4u;

    const int split = xcd_swizzle(blockIdx.x, gridDim.x);
    if (split >= a.nsplit) return;
    const int rpi = a.H / ROWS, nruns = a.B * rpi;
    const int run_begin = (int)((long)nruns * split / a.nsplit), run_end = (int)((long)nruns * (split + 1) / a.nsplit);

    // zero halo groups of the activated rows and the margins of the dy2 ring, for the kernel's life
    for (int e = tid; e < 2 * CI * NSLOT * 2; e += NTHR) sX[(e / 2) * XG + (e % 2) * (XG - 1)] = u32x4{0u, 0u, 0u, 0u};
    for (int e = tid; e < 2 * 2 * NSLOT * 8; e += NTHR) sIn[(e / 8) * IW + (e % 8 < 4 ? e % 8 : IW - 8 + e % 8)] = u32x4{0u, 0u, 0u, 0u};

    float bs_md = 0.f, bs_mx = 0.f;

    if (wave_u < 4) {
        // =========================== waves 0-3: dy2 staging and the weight gradient ===========================
        const int sp = wave_u;                            // segment pair (K split) of this wave's weight-gradient work
        const int dc0 = wave_u * 4, cg = wave_u >> 1, ch = wave_u & 1;      // staging: dy2 channels dc0 .. dc0 + 3 = half ch of channel group cg; lane = pixels 4 lane .. 4 lane + 3
        const bool want_bias = a.bslab != nullptr;
        f32x4 rd[4], ry[4];
        bool d_in = false;
        float dtc[4][6];                                  // (mean, invstd, gamma invstd, beta, mean(d), mean(d x_hat)) of this wave's dy2 channels
        auto ld4 = [](__amdgpu_buffer_rsrc_t rs, uint32_t off) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0)); };
        auto load_d = [&](int b, int gy, f32x4 (&dd)[4], f32x4 (&yy)[4], bool& ok) {      // every wave-instruction a 1-KiB row of one channel
            ok = (unsigned)gy < (unsigned)a.H;
            const __amdgpu_buffer_rsrc_t rsd = make_rsrc(a.dact + (size_t)b * 16 * HW, 16u * HW4);
            const __amdgpu_buffer_rsrc_t rsy = make_rsrc(a.y2 + (size_t)b * 16 * HW, 16u * HW4);
            const uint32_t off = (uint32_t)(dc0 * HW + gy * W + lane * 4) * 4u;
#pragma unroll
            for (int i = 0; i < 4; ++i) dd[i] = ld4(rsd, ok ? off + (uint32_t)i * HW4 : kOob);
#pragma unroll
            for (int i = 0; i < 4; ++i) yy[i] = ld4(rsy, ok ? off + (uint32_t)i * HW4 : kOob);
        };
        // dy2 = sc (d - k2 - x_hat k3), d = g or slope g by the sign of the BatchNorm output (conv_split_wrw_row.hpp: store_d); rows outside
        // the image are zero.  buf < 0: a halo row, which the weight gradient must not see
        auto store_d = [&](f32x4 (&dd)[4], f32x4 (&yy)[4], bool ok, int slot, int buf) {
            float v[4][4];
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
            // the ring: this wave's four channels are two dwords of every pixel's 16-byte unit (8 channels)
            const int base = (cg * NSLOT + slot) * IW + 4 + lane * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned q00, q01, q10, q11;
                conv_split2h(v[0][k] * sc_d, v[1][k] * sc_d, q00, q01);
                conv_split2h(v[2][k] * sc_d, v[3][k] * sc_d, q10, q11);
                *reinterpret_cast<uint2*>(reinterpret_cast<unsigned*>(&sIn[base + k]) + ch * 2) = make_uint2(q00, q10);
                *reinterpret_cast<uint2*>(reinterpret_cast<unsigned*>(&sIn[PIECE + base + k]) + ch * 2) = make_uint2(q01, q11);
            }
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
        constexpr unsigned kOnes = 0x3C003C00u;           // two fp16 1.0
        const f16x8 ones = __builtin_bit_cast(f16x8, u32x4{kOnes, kOnes, kOnes, kOnes});

        for (int run = run_begin; run < run_end; ++run) {
            const int b = run / rpi, r0 = (run % rpi) * ROWS;
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
                const int s1 = s0 + 1 >= NSLOT ? s0 + 1 - NSLOT : s0 + 1, s2 = s1 + 1 >= NSLOT ? s1 + 1 - NSLOT : s1 + 1;
                const u32x4* sDb = sD + buf * D_UNITS;
                // ---- dy2 row t against the activated rows t - 1, t, t + 1 (conv_hrwrw_body's contract) ----
#pragma unroll
                for (int sgi = 0; sgi < 2; ++sgi) {
                    const int gq = (sp * 2 + sgi) * 4 + kq;       // this lane's 8-pixel group of the row
                    f16x8 af[2];
#pragma unroll
                    for (int p = 0; p < 2; ++p) af[p] = __builtin_bit_cast(f16x8, sDb[(p * 16 + j) * NG + gq]);
                    if (want_bias) {
                        accb = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1], ones, accb, 0, 0, 0);
                        accb = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0], ones, accb, 0, 0, 0);
                    }
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        const int slot = ky == 0 ? s0 : (ky == 1 ? s1 : s2);
                        f16x8 bf[3][2];                    // [shift kx][piece]
#pragma unroll
                        for (int p = 0; p < 2; ++p) {
                            const int u = ((p * CI + j) * NSLOT + slot) * XG + gq + 1;
                            const u32x4 c = sX[u];
                            const unsigned cl3 = reinterpret_cast<const unsigned*>(&sX[u - 1])[3];
                            const unsigned cr0 = reinterpret_cast<const unsigned*>(&sX[u + 1])[0];
                            const unsigned t01 = __builtin_amdgcn_alignbit(c[1], c[0], 16), t12 = __builtin_amdgcn_alignbit(c[2], c[1], 16);
                            const unsigned t23 = __builtin_amdgcn_alignbit(c[3], c[2], 16);
                            const unsigned tE0 = __builtin_amdgcn_alignbit(c[0], cl3, 16), t3E = __builtin_amdgcn_alignbit(cr0, c[3], 16);
                            bf[0][p] = __builtin_bit_cast(f16x8, u32x4{tE0, t01, t12, t23});
                            bf[1][p] = __builtin_bit_cast(f16x8, c);
                            bf[2][p] = __builtin_bit_cast(f16x8, u32x4{t01, t12, t23, t3E});
                        }
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            f32x4 c = acc[ky * 3 + kx];
                            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1], bf[kx][0], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0], bf[kx][1], c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0], bf[kx][0], c, 0, 0, 0);
                            acc[ky * 3 + kx] = c;
                        }
                    }
                }
                __syncthreads();                          // every wave is done with row t - 1 of both rings and with dy2 row t
                if (more) store_d(rd, ry, d_in, s0, buf);
                s0 = s1; buf ^= 1;
                __syncthreads();
            }
        }

        // ---- sum the four K-split partials through LDS (fixed order), as conv_hrwrw_body ----
        float* red = reinterpret_cast<float*>(sX);         // [slot][10][4][64]; the staging image is dead (the loop ended with a barrier)
#pragma unroll
        for (int s = 2; s >= 1; s >>= 1) {
            if (sp >= s && sp < 2 * s) {
                float* p = red + (size_t)(sp - s) * 10 * 256 + lane;
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) p[(t * 4 + r) * 64] = acc[t][r];
#pragma unroll
                for (int r = 0; r < 4; ++r) p[(36 + r) * 64] = accb[r];
            }
            __syncthreads();
            if (sp < s) {
                const float* p = red + (size_t)sp * 10 * 256 + lane;
#pragma unroll
                for (int t = 0; t < 9; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t][r] += p[(t * 4 + r) * 64];
#pragma unroll
                for (int r = 0; r < 4; ++r) accb[r] += p[(36 + r) * 64];
            }
            __syncthreads();
        }
        if (sp == 0) {
            // lane (j, kq), register r: co = kq * 4 + r, ci = j; the slab is [tap][16][16]
            float* slab = a.slab + (size_t)split * 9 * 16 * CI;
            float chk = 0.f;
            const float inv = inv_d * inv_x;               // exact: powers of two
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                note_nonfinite(chk, acc[t]);
#pragma unroll
                for (int r = 0; r < 4; ++r) slab[((size_t)t * 16 + kq * 4 + r) * CI + j] = acc[t][r] * inv;
            }
            report_nonfinite(a.err, chk, UAPS_ERR_WRW_NONFINITE);
            if (want_bias && j == 0) {
                // (a vector register of its own: from the scalar pair (scale, 1 / scale) the packed multiply took 1 / scale by a low-half
                // op_sel, which tools/isa_lint.py keeps out of the library: DESIGN.md section 4)
                float inv_b = inv_d;
                asm volatile("" : "+v"(inv_b));
#pragma unroll
                for (int r = 0; r < 4; ++r) a.bslab[(size_t)split * 16 + kq * 4 + r] = accb[r] * inv_b;
            }
        }
    } else {
        // =========================== waves 4-7: y1 staging, the input gradient and the BatchNorm-backward sums ===========================
        const int wg = wave_u - 4;
        const int xc0 = wg * NXL;                         // staging: y1 channels xc0 .. xc0 + 3, lane = pixels 4 lane .. 4 lane + 3
        const float out_scale_a = inv_d, out_scale_w = a.wscale[1];      // (the input scale is sc_d: lz.bound bounds dy2 for both contractions)

        // input-gradient weight fragments, once: lane (n = j, k-group kq) of step s holds k-group q = 4 s + kq = (tap q / 2, channel group q % 2)
        u32x4 bfr[NSTEP][2];
        int kxo[NSTEP], kyv[NSTEP];
        {
            const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(a.wp, (uint32_t)(2 * 9) * a.CGP * 16u * 16u);
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) {
                const int q = 4 * s + kq, tap = q / 2, cgq = q % 2;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const uint32_t off = q < NQ ? (uint32_t)(((p * 9 + tap) * a.CGP + cgq) * 16 + j) * 16u : kOob;
                    bfr[s][p] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (int)off, 0, 0);
                }
                const int qq = q < NQ ? q : 0;                // padded k-groups meet zero weights
                kxo[s] = (qq % 2) * CGU + (qq / 2) % 3; kyv[s] = (qq / 2) / 3;
            }
        }
        int abase[MW];
#pragma unroll
        for (int m = 0; m < MW; ++m) abase[m] = (wg * MW + m) * 16 + j + XS;

        f32x4 rx[NXL], xa[NXL], xb[NXL];
        f32x2 cf[NXL];
        float bs_mu[NXL], bs_is[NXL], bs_sc[NXL], bs_sh[NXL];
        bool x_in = false;
        auto ld4 = [](__amdgpu_buffer_rsrc_t rs, uint32_t off) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0)); };
        auto load_x = [&](int b, int gy, f32x4 (&dst)[NXL], bool& ok) {
            ok = (unsigned)gy < (unsigned)a.H;
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.y1 + (size_t)b * CI * HW, (uint32_t)CI * HW4);
            const uint32_t off = (uint32_t)(xc0 * HW + gy * W + lane * 4) * 4u;
#pragma unroll
            for (int i = 0; i < NXL; ++i) dst[i] = ld4(rs, ok ? off + (uint32_t)i * HW4 : kOob);
        };
        auto store_x = [&](f32x4 (&src)[NXL], bool ok, int slot) {
#pragma unroll
            for (int i = 0; i < NXL; ++i) {
                asm volatile("" : "+v"(src[i]));
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {             // leaky_relu(fma(y, scale, shift)); rows outside the image stay zero
                    const float z = __builtin_fmaf(src[i][k], cf[i].x, cf[i].y);
                    v[k] = ok ? __builtin_fmaxf(z, z * a.slope) : 0.f;
                }
                unsigned a0, a1, b0, b1;
                conv_split2h(v[0] * sc_x, v[1] * sc_x, a0, a1);
                conv_split2h(v[2] * sc_x, v[3] * sc_x, b0, b1);
                const int c = xc0 + i;
                unsigned* p0 = reinterpret_cast<unsigned*>(&sX[(c * NSLOT + slot) * XG + 1]) + lane * 2;
                unsigned* p1 = reinterpret_cast<unsigned*>(&sX[((CI + c) * NSLOT + slot) * XG + 1]) + lane * 2;
                *reinterpret_cast<uint2*>(p0) = make_uint2(a0, b0);
                *reinterpret_cast<uint2*>(p1) = make_uint2(a1, b1);
            }
        };

        for (int run = run_begin; run < run_end; ++run) {
            const int b = run / rpi, r0 = (run % rpi) * ROWS;
            const int grp = b / a.Bg;
            float st_s[NXL][4], st_q[NXL][4];             // [channel][row % 4]: the four waves of bn_bwd_sums_max_kernel's block
#pragma unroll
            for (int i = 0; i < NXL; ++i) {
                const int c = xc0 + i;
                const float2 t = a.xf[(size_t)grp * CI + c];
                cf[i] = f32x2{t.x, t.y};
                bs_mu[i] = a.bs_mean[grp * CI + c]; bs_is[i] = a.bs_invstd[grp * CI + c];
                bs_sc[i] = a.bs_gamma[c] * bs_is[i]; bs_sh[i] = a.bs_beta[c];
#pragma unroll
                for (int v = 0; v < 4; ++v) { st_s[i][v] = 0.f; st_q[i][v] = 0.f; }
            }
            // y1 rows r0 - 1, r0, r0 + 1 into slots 0, 1, 2: all fetches in flight together
            {
                f32x4 ra[NXL];
                bool oka, okb;
                load_x(b, r0 - 1, ra, oka);
                load_x(b, r0, xa, okb);
                load_x(b, r0 + 1, xb, x_in);
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
                if (more) load_x(b, t + 2, rx, x_in);
                const int s1 = s0 + 1 >= NSLOT ? s0 + 1 - NSLOT : s0 + 1, s2 = s1 + 1 >= NSLOT ? s1 + 1 - NSLOT : s1 + 1;

                // ---- d(act1) row t, this wave's four 16-pixel tiles: conv_hr16_body's k order and products ----
                int aoff[NSTEP];
#pragma unroll
                for (int s = 0; s < NSTEP; ++s) aoff[s] = kxo[s] + (kyv[s] == 0 ? s0 : (kyv[s] == 1 ? s1 : s2)) * IW;
                f32x4 gacc[MW];
#pragma unroll
                for (int m = 0; m < MW; ++m) gacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
                constexpr int NUN = NSTEP * MW;
                u32x4 af[2][2];
                auto read_a = [&](int u, u32x4 (&dst)[2]) {
                    const int s = u / MW, m = u % MW;
#pragma unroll
                    for (int p = 0; p < 2; ++p) dst[p] = sIn[p * PIECE + abase[m] + aoff[s]];
                };
                read_a(0, af[0]);
#pragma unroll
                for (int u = 0; u < NUN; ++u) {
                    const int s = u / MW, m = u % MW;
                    if (u + 1 < NUN) read_a(u + 1, af[(u + 1) & 1]);
                    const auto Hf = [](const u32x4& v) { return __builtin_bit_cast(f16x8, v); };
                    f32x4 c = gacc[m];
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Hf(af[u & 1][1]), Hf(bfr[s][0]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Hf(af[u & 1][0]), Hf(bfr[s][1]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Hf(af[u & 1][0]), Hf(bfr[s][0]), c, 0, 0, 0);
                    gacc[m] = c;
                    if (u + 1 < NUN) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      // next unit's DS reads first ...
                    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                       // ... then this unit's MFMAs
                }
                // lane (j, kq) holds pixels kq * 4 .. kq * 4 + 3 of channel j of every tile
                float chk = 0.f;
#pragma unroll
                for (int m = 0; m < MW; ++m) {
                    f32x4 v = gacc[m];
                    v *= out_scale_a; v *= out_scale_w;   // exact: powers of two
                    v += 0.f;                             // (the row kernel adds its absent bias)
                    note_nonfinite(chk, v);
                    *reinterpret_cast<f32x4*>(&sG[j * GS + (wg * MW + m) * 16 + kq * 4]) = v;
                }
                report_nonfinite(a.err, chk, UAPS_ERR_CONV_NONFINITE);
                __syncthreads();                          // every wave is done with row t - 1 of both rings; d(act1) row t is complete

                // ---- d(act1) row t out, and the BatchNorm-backward sums of (d(act1), y1) row t: bn_bwd_sums_max_kernel per element ----
#pragma unroll
                for (int i = 0; i < NXL; ++i) {
                    const f32x4 gv = *reinterpret_cast<const f32x4*>(&sG[(xc0 + i) * GS + lane * 4]);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, gv), rs_g, (int)((uint32_t)((xc0 + i) * HW + t * W + lane * 4) * 4u), 0, 0);
                    // that kernel's thread (wave v, lane) sums rows v, v + 4, v + 8, v + 12 of the 16-row chunk at this lane's four columns, in
                    // this order: slot 0 of the rotating set is row t's wave
                    float cs = st_s[i][0], cq = st_q[i][0];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float yc = xa[i][e] - bs_mu[i], z = yc * bs_sc[i] + bs_sh[i];
                        const float d = z > 0.f ? gv[e] : gv[e] * a.slope, xh = yc * bs_is[i];
                        cs += d; cq += d * xh;
                        bs_md = __builtin_fmaxf(bs_md, __builtin_fabsf(d)); bs_mx = __builtin_fmaxf(bs_mx, __builtin_fabsf(xh));
                    }
#pragma unroll
                    for (int v = 0; v < 3; ++v) { st_s[i][v] = st_s[i][v + 1]; st_q[i][v] = st_q[i][v + 1]; }
                    st_s[i][3] = cs; st_q[i][3] = cq;
                }
                if (more) store_x(rx, x_in, s0);
#pragma unroll
                for (int i = 0; i < NXL; ++i) { xa[i] = xb[i]; xb[i] = rx[i]; }
                s0 = s1;
                __syncthreads();
            }
            // one part per (channel, run) in block_sum2's order (norm_act.hip): the lane butterfly of each of the four waves, then the waves
            // in turn -- the part bn_bwd_sums_max_kernel writes for this 4096-float chunk, bit for bit
#pragma unroll
            for (int i = 0; i < NXL; ++i) {
                float s = 0.f, q = 0.f;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    float sv = st_s[i][v], qv = st_q[i][v];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) { sv += __shfl_xor(sv, o, 64); qv += __shfl_xor(qv, o, 64); }
                    s = v == 0 ? sv : s + sv; q = v == 0 ? qv : q + qv;
                }
                if (lane == 0) a.partials[((size_t)(xc0 + i) * a.B + b) * rpi + r0 / ROWS] = make_float2(s, q);
            }
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
    // the slabs of this layer's weight-gradient plan ([split][tap][16][16] + [split][16]): workspace and reduction are the plan's
    size_t need = 0;
    const int rc = uaps_conv_wrw_workspace_bytes(B, Cin, Cout, H, W, ks, cfg, &need);
    if (rc) return rc;
    constexpr int CoutS = 16, CinS = 16;
    const size_t per_split = ((size_t)9 * CoutS * CinS + CoutS) * sizeof(float);
    if (need == 0 || need % per_split) return UAPS_ENOFORM;
    const int nsplit = (int)(need / per_split);
    if (ws_bytes < need) return UAPS_EWORKSPACE;
    // d(act2), y2 and y1 in, d(act1) out: each once
    uaps::account_bytes(4.0 * B * H * W * (3.0 * Cout + 1.0 * Cin));
    uaps::MidBwdArgs a{};
    a.dact = dact; a.y2 = y2; a.coef = coef; a.dt_slope = slope2; a.dt_Bg = B / groups2;
    a.y1 = y1; a.xf = (const float2*)xf; a.slope = slope; a.Bg = B / groups;
    // the packed input-gradient weights (uaps_conv_pack_weights): the exact GEMM layout, three bf16 pieces, a header, two fp16 pieces
    const int CGP = uaps::split_cgroups(Cout);
    const float* split_w = wb + (size_t)9 * ((Cout + 7) / 8 * 8) * ((Cin + 15) / 16 * 16);
    const size_t piece = (size_t)9 * CGP * ((Cin + 15) / 16 * 16) * 4;
    a.wscale = split_w + 3 * piece + 16;
    a.wp = split_w + 3 * piece + uaps::kH16Header;
    a.CGP = CGP;
    a.g = g;
    a.slab = (float*)ws; a.nsplit = nsplit;
    a.bslab = want_bias ? a.slab + (size_t)nsplit * 9 * CoutS * CinS : nullptr;
    a.dy_bound = dy_bound; a.dy_mul = dy_mul; a.in_bound = x_bound; a.in_mul = x_mul;
    a.bs_mean = save_mean; a.bs_invstd = save_invstd; a.bs_gamma = gamma; a.bs_beta = beta;
    a.partials = (float2*)partials; a.bs_max = maxes;
    a.err = uaps::error_word();
    a.B = B; a.H = H;
    const unsigned grid = (unsigned)((nsplit + 7) / 8 * 8);
    UAPS_LAUNCH_MAIN(uaps::mid_bwd_row_kernel, dim3(grid), dim3(512), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
