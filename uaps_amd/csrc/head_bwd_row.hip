// The backward of a decoder's class convolution (out_conv: 3x3, 16 -> <= 4 channels, UAPS_unet.py:138) on 256-pixel-wide maps and the
// BatchNorm-backward sums of the layer in front of it, ONE pass (include/uaps_hip.h: uaps_head_bwd_fused).
//
// Until now three HBM-bound launches ran back to back here and read the same two tensors: the input gradient g = W^T (*) d logits
// (conv_fwd_kernel<3, 8, 32, 16, 4, 4, 1>: reads d logits, writes g), the weight gradient (conv_hrwrw_bn_kernel<1>: reads d logits and
// the raw output y of the convolution in front) and the sums pass of that layer's BatchNorm backward (bn_bwd_sums_max_kernel: reads g
// and y) -- 4.6 tensors of 16 channels moved where 2.25 are needed: d logits (a quarter) and y in, g out.
//
// The kernel is conv_hrwrw_body<1, XF = true> (conv_split_wrw_row.hpp) with two more consumers of its staged rows.  A workgroup owns
// runs of 16 rows of one image at full width and walks down them one row per step; per step it fetches ONE new row of y (16
// channels) and ONE of d logits (4 channels), two rows ahead of the row it works on, and for row t
//   * contracts d logits row t with the activated rows t - 1, t, t + 1 of x = leaky_relu(fma(y, scale, shift)) into the nine tap
//     accumulators of dW (and the bias gradient): conv_hrwrw_body's arithmetic, order and slabs, bit for bit.  The fp16 pieces
//     of d logits are split from the fp32 ring when the fragment is read (<= 4 channels: no second staged image of it);
//   * forms g row t from the fp32 ring of d logits rows t - 1, t, t + 1 with v_mfma_f32_16x16x4_f32, one instruction per tap in
//     tap order from the fp32 GEMM layout at the front of the packed input-gradient weights: conv_fwd_body's k order, so g is
//     bit-identical to that kernel's;
//   * hands g row t through LDS from the matrix layout (channel = lane % 16) to the staging layout (a wave = 4 channels, a lane = 4
//     consecutive pixels), where the raw y row t still sits in the registers it was fetched into two steps earlier: g goes to
//     memory as whole 1-KiB rows, and bn_bwd_sums_max_kernel's per-element arithmetic runs on (g, y) in registers.
// One float2 (sum d, sum d x_hat) per (channel, image, run) goes to `partials`, summed in the order of bn_bwd_sums_max_kernel's block for
// the same 4096 floats (a run IS that kernel's chunk), so the BatchNorm coefficients are bit-identical too; the two maxima go to
// `bs_max` (uaps_bn_act_bwd_finalize's inputs).  No float atomics; two launches give the same bits.
//
// LDS: activated rows 52224 B + d logits ring 12672 B + g exchange 16640 B = 81536 B: two workgroups per CU.
#include "../../include/uaps_hip.h"
#include "conv_kernels.hpp"
#include "conv_split.hpp"
#include "hints.hpp"

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
    constexpr int WIDTH = 256, NG = WIDTH / 8, XG = NG + 2, NSLOT = 3, ROWS = 16, CI = 16, NTHR = 256, NXL = 4;
    constexpr int XCH = NSLOT * XG;
    constexpr int X_UNITS = 2 * CI * XCH;
    constexpr int DW = WIDTH + 8;                         // floats of a d-logits ring row: 4 of margin either side (columns -1 and 256 are zero)
    constexpr int GS = WIDTH + 4;                         // channel stride of the g exchange image
    constexpr int RED_FLOATS = 2 * 10 * 256;
    static_assert(RED_FLOATS / 4 <= X_UNITS, "the reduction scratch fits the input image");

    __shared__ __attribute__((aligned(16))) u32x4 sX[X_UNITS];             // [piece][ci][slot][group]
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

    const int split = xcd_swizzle(blockIdx.x, gridDim.x);
    if (split >= a.nsplit) return;
    const int rpi = a.H / ROWS, nruns = a.B * rpi;
    const int run_begin = (int)((long)nruns * split / a.nsplit), run_end = (int)((long)nruns * (split + 1) / a.nsplit);
    const bool want_bias = a.bslab != nullptr;

    // zero halo groups of the activated rows and the margins of the d-logits ring, for the kernel's life
    for (int e = tid; e < 2 * CI * NSLOT * 2; e += NTHR) sX[(e / 2) * XG + (e % 2) * (XG - 1)] = u32x4{0u, 0u, 0u, 0u};
    for (int e = tid; e < 4 * NSLOT * 8; e += NTHR) sDf[(e / 8) * DW + (e % 8 < 4 ? e % 8 : WIDTH + e % 8)] = 0.f;

    // input-gradient weights: lane (n = j, k = kq) of tap t holds wp[t][kq][j]
    float bw[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) bw[t] = a.wp[(t * 4 + kq) * 16 + j];

    // ---- staging: lane = pixels 4 lane .. 4 lane + 3 of y channels 4 wave .. 4 wave + 3 and of d-logits channel `wave` ----
    f32x4 rx[NXL], xa[NXL], xb[NXL], rd;
    f32x2 cf[NXL];
    float bs_mu[NXL], bs_is[NXL], bs_sc[NXL], bs_sh[NXL];
    bool x_in = false;
    const int xc0 = wave_u * NXL;
    auto ld4 = [](__amdgpu_buffer_rsrc_t rs, uint32_t off) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0)); };
    auto load_x = [&](int b, int gy, f32x4 (&dst)[NXL], bool& ok) {
        ok = (unsigned)gy < (unsigned)a.H;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.y + (size_t)b * CI * HW, (uint32_t)CI * HW4);
        const uint32_t off = (uint32_t)(xc0 * HW + gy * W + lane * 4) * 4u;
#pragma unroll
        for (int i = 0; i < NXL; ++i) dst[i] = ld4(rs, ok ? off + (uint32_t)i * HW4 : kOob);
    };
    auto load_d = [&](int b, int gy, f32x4& dst) {        // rows outside the image and absent channels read zeros
        const bool ok = (unsigned)gy < (unsigned)a.H && wave_u < a.Cout;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.dlog + (size_t)b * a.Cout * HW, (uint32_t)a.Cout * HW4);
        dst = ld4(rs, ok ? (uint32_t)(wave_u * HW + gy * W + lane * 4) * 4u : kOob);
    };
    auto store_x = [&](f32x4 (&src)[NXL], bool ok, int slot) {
#pragma unroll
        for (int i = 0; i < NXL; ++i) {
            asm volatile("" : "+v"(src[i]));
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {                 // leaky_relu(fma(y, scale, shift)); rows outside the image stay zero
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
    auto store_d = [&](f32x4& src, int slot) {
        asm volatile("" : "+v"(src));
        *reinterpret_cast<f32x4*>(&sDf[(wave_u * NSLOT + slot) * DW + 4 + lane * 4]) = src;
    };

    f32x4 acc[9];
    f32x4 accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr unsigned kOnes = 0x3C003C00u;               // two fp16 1.0
    const f16x8 ones = __builtin_bit_cast(f16x8, u32x4{kOnes, kOnes, kOnes, kOnes});
    float bs_md = 0.f, bs_mx = 0.f;

    for (int run = run_begin; run < run_end; ++run) {
        const int b = run / rpi, r0 = (run % rpi) * ROWS;
        const int grp = b / a.Bg;
        float st_s[NXL][4], st_q[NXL][4];                 // [channel][row % 4]: the four waves of bn_bwd_sums_max_kernel's block
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
        // rows r0 - 1, r0, r0 + 1 of both operands into slots 0, 1, 2: all fetches in flight together
        {
            f32x4 ra[NXL], da, db;
            bool oka, okb;
            load_x(b, r0 - 1, ra, oka);
            load_x(b, r0, xa, okb);
            load_x(b, r0 + 1, xb, x_in);
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
            if (more) { load_x(b, t + 2, rx, x_in); load_d(b, t + 2, rd); }
            const int s1 = s0 + 1 >= NSLOT ? s0 + 1 - NSLOT : s0 + 1, s2 = s1 + 1 >= NSLOT ? s1 + 1 - NSLOT : s1 + 1;

            // ---- weight gradient: d-logits row t against the activated rows t - 1, t, t + 1 (conv_hrwrw_body's contract) ----
#pragma unroll
            for (int sgi = 0; sgi < 2; ++sgi) {
                const int gq = (sp * 2 + sgi) * 4 + kq;   // this lane's 8-pixel group of the row
                f16x8 af[2];
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
                if (want_bias) {
                    accb = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1], ones, accb, 0, 0, 0);
                    accb = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0], ones, accb, 0, 0, 0);
                }
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int slot = ky == 0 ? s0 : (ky == 1 ? s1 : s2);
                    f16x8 bf[3][2];                        // [shift kx][piece]
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

            // ---- g row t out, and the BatchNorm-backward sums of (g, y) row t: norm_act.hip's dpre / bn_bwd_sums_max_kernel per element ----
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
            if (more) { store_x(rx, x_in, s0); store_d(rd, s0); }
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

    // ---- sum the four K-split partials through LDS (fixed order), as conv_hrwrw_body ----
    float* red = reinterpret_cast<float*>(sX);             // [slot][10][4][64]; the staging image is dead (the loop ended with a barrier)
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
    block_amax_to(a.bs_max, bs_md, sG);                    // (sG is dead; every thread of the workgroup gets here)
    block_amax_to(a.bs_max + UAPS_BOUND_FLOATS, bs_mx, sG + 16);
    if (sp != 0) return;
    // lane (j, kq), register r: co = kq * 4 + r, ci = j; the slab is [tap][CoutS][16]
    float* slab = a.slab + (size_t)split * 9 * a.CoutS * CI;
    float chk = 0.f;
    const float inv = inv_d * inv_x;                       // exact: powers of two
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        note_nonfinite(chk, acc[t]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = kq * 4 + r;
            if (co < a.CoutS) slab[((size_t)t * a.CoutS + co) * CI + j] = acc[t][r] * inv;
        }
    }
    report_nonfinite(a.err, chk, UAPS_ERR_WRW_NONFINITE);
    if (want_bias && j == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (kq * 4 + r < a.CoutS) a.bslab[(size_t)split * a.CoutS + kq * 4 + r] = accb[r] * inv_d;
    }
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
    // the slabs of this layer's weight-gradient plan (the exact-N layout [split][tap][4][16] + [split][4]): workspace and reduction are the plan's
    size_t need = 0;
    const int rc = uaps_conv_wrw_workspace_bytes(B, Cin, Cout, H, W, ks, cfg, &need);
    if (rc) return rc;
    constexpr int CoutS = 4, CinS = 16;
    const size_t per_split = ((size_t)9 * CoutS * CinS + CoutS) * sizeof(float);
    if (need == 0 || need % per_split) return UAPS_ENOFORM;
    const int nsplit = (int)(need / per_split);
    if (ws_bytes < need) return UAPS_EWORKSPACE;
    // d logits and y in, g out: each once
    uaps::account_bytes(4.0 * B * H * W * ((double)Cout + 2.0 * Cin));
    uaps::HeadBwdArgs a{};
    a.dlog = dlogits; a.y = y; a.wp = wb; a.g = g;
    a.xf = (const float2*)xf; a.slope = slope; a.Bg = B / groups;
    a.slab = (float*)ws; a.nsplit = nsplit; a.CoutS = CoutS;
    a.bslab = want_bias ? a.slab + (size_t)nsplit * 9 * CoutS * CinS : nullptr;
    a.dy_bound = dy_bound; a.dy_mul = dy_mul; a.in_bound = x_bound; a.in_mul = x_mul;
    a.bs_mean = save_mean; a.bs_invstd = save_invstd; a.bs_gamma = gamma; a.bs_beta = beta;
    a.partials = (float2*)partials; a.bs_max = maxes;
    a.err = uaps::error_word();
    a.B = B; a.Cout = Cout; a.H = H;
    const unsigned grid = (unsigned)((nsplit + 7) / 8 * 8);
    UAPS_LAUNCH_MAIN(uaps::head_bwd_row_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
