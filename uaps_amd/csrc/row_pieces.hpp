// The shared pieces of the full-width-row kernels of the 256-wide level: conv_hrwrw_body (conv_split_wrw_row.hpp) and the three fused
// backward passes head_bwd_row.hip, mid_bwd_row.hip and up_bwd_row.hip.  A workgroup of these kernels owns runs of 16 rows of one
// image and walks down them one row per step over rings of three row slots in LDS; the kernels are the wave-role bodies that say
// which piece runs when and between which workgroup barriers, the pieces are the arithmetic.  Every piece exists ONCE: where a fused
// pass promises the bits of an un-fused kernel, both run the same text.
//
// Every piece is inlined into its caller; what differs between the callers is a template argument or a value that is a constant where
// the caller has it as one -- no piece has a run-time switch of its own.
#pragma once
#include "conv_kernels.hpp"
#include "conv_split.hpp"
#include "hints.hpp"

namespace uaps {

// The geometry of a row walk over CI_ staged input channels
template <int CI_>
struct RowGeom {
    static constexpr int WIDTH = 256, ROWS = 16, NSLOT = 3, CI = CI_;
    static constexpr int NG = WIDTH / 8, XG = NG + 2;                 // 8-pixel groups of a row; with a zero group either side (the image edge)
    static constexpr int X_UNITS = 2 * CI * NSLOT * XG;               // the activated rows [piece][ci][slot][group]
    static constexpr int D_UNITS = 2 * 16 * NG;                       // one pixel-grouped dy row [piece][co][group]
    static constexpr int IW = WIDTH + 8, CGU = NSLOT * IW, PIECE = 2 * CGU, XS = 3;      // the dy ring: conv_hr16_body's image with three row slots
    static constexpr int NQ = 9 * 2, NSTEP = (NQ + 3) / 4, MW = 4;    // input gradient: k-groups (tap, channel group), steps of four, tiles per wave
    static constexpr int GS = WIDTH + 4;                              // channel stride of an exchange row
    static constexpr int NXL = 4;                                     // channels a staging wave fetches per row
};

// ---- I. run partition, ring-slot rotation, the zeros that last the kernel's life ----
struct RowRuns { int split, rpi, begin, end; };
// false: this workgroup has no runs
template <class G>
__device__ __forceinline__ bool row_runs(int B, int H, int nsplit, RowRuns& r) {
    r.split = xcd_swizzle(blockIdx.x, gridDim.x);
    if (r.split >= nsplit) return false;
    r.rpi = H / G::ROWS;
    const int nruns = B * r.rpi;
    r.begin = (int)((long)nruns * r.split / nsplit); r.end = (int)((long)nruns * (r.split + 1) / nsplit);
    return true;
}
// s0 is the slot of row t - 1; rows t, t + 1 follow cyclically
template <class G>
__device__ __forceinline__ void ring_slots(int s0, int& s1, int& s2) {
    s1 = s0 + 1 >= G::NSLOT ? s0 + 1 - G::NSLOT : s0 + 1; s2 = s1 + 1 >= G::NSLOT ? s1 + 1 - G::NSLOT : s1 + 1;
}
// the halo groups (image columns -8 .. -1 and 256 .. 263) of every (piece, channel, slot) of the activated rows
template <class G, int NTHR>
__device__ __forceinline__ void zero_x_halo(u32x4* sX, int tid) {
    for (int e = tid; e < 2 * G::CI * G::NSLOT * 2; e += NTHR) sX[(e / 2) * G::XG + (e % 2) * (G::XG - 1)] = u32x4{0u, 0u, 0u, 0u};
}
// the margins of every row slot of the dy ring (image columns -4 .. -1 and 256 .. 259)
template <class G, int NTHR>
__device__ __forceinline__ void zero_ring_margins(u32x4* sIn, int tid) {
    for (int e = tid; e < 2 * 2 * G::NSLOT * 8; e += NTHR) sIn[(e / 8) * G::IW + (e % 8 < 4 ? e % 8 : G::IW - 8 + e % 8)] = u32x4{0u, 0u, 0u, 0u};
}

// ---- the 4-channel row loader of D and E: every wave-instruction a 1-KiB row of one channel of a 16-channel tensor `t`; lane = pixels
// 4 lane .. 4 lane + 3 of channels c0 .. c0 + 3.  A row outside the image reads zeros (no memory access); returns whether it is inside ----
template <class G>
__device__ __forceinline__ bool load_rows4(const float* t, int b, int gy, int H, int c0, int lane, f32x4 (&dst)[4]) {
    const int HW = H * G::WIDTH;
    const uint32_t HW4 = (uint32_t)HW * 4u;
    const bool ok = (unsigned)gy < (unsigned)H;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(t + (size_t)b * 16 * HW, 16u * HW4);
    const uint32_t off = (uint32_t)(c0 * HW + gy * G::WIDTH + lane * 4) * 4u;
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(ok ? off + (uint32_t)i * HW4 : kOob), 0, 0));
    return ok;
}

// ---- A. tap contraction: one dy row fragment `af` (both pieces) against the activated rows t - 1, t, t + 1 (ring slots slot_of(0 .. 2),
// a callable: each caller keeps its own way from s0 to the three slots, evaluated where the row is read) of input channel `ci` at the
// lane's 8-pixel group gq, into the nine tap accumulators; with `bias` the fragment also meets a row of ones.  The column taps come
// from the aligned fragment and the neighbour groups' boundary dwords.  conv_hrwrw_body's contraction ----
template <class G, class SlotOf>
__device__ __forceinline__ void tap_contract(const u32x4* sX, const f16x8 (&af)[2], int ci, int gq, const SlotOf& slot_of, bool bias,
                                             f32x4 (&acc)[9], f32x4& accb) {
    constexpr unsigned kOnes = 0x3C003C00u;               // two fp16 1.0
    const f16x8 ones = __builtin_bit_cast(f16x8, u32x4{kOnes, kOnes, kOnes, kOnes});
    if (bias) {
        accb = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1], ones, accb, 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0], ones, accb, 0, 0, 0);
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int slot = slot_of(ky);
        f16x8 bf[3][2];                                   // [shift kx][piece]
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int u = ((p * G::CI + ci) * G::NSLOT + slot) * G::XG + gq + 1;
            const u32x4 c = sX[u];
            const unsigned cl3 = reinterpret_cast<const unsigned*>(&sX[u - 1])[3];      // pixels x - 2, x - 1 of the group's first pixel
            const unsigned cr0 = reinterpret_cast<const unsigned*>(&sX[u + 1])[0];      // pixels x + 8, x + 9
            const unsigned t01 = __builtin_amdgcn_alignbit(c[1], c[0], 16), t12 = __builtin_amdgcn_alignbit(c[2], c[1], 16);
            const unsigned t23 = __builtin_amdgcn_alignbit(c[3], c[2], 16);
            const unsigned tE0 = __builtin_amdgcn_alignbit(c[0], cl3, 16), t3E = __builtin_amdgcn_alignbit(cr0, c[3], 16);
            bf[0][p] = __builtin_bit_cast(f16x8, u32x4{tE0, t01, t12, t23});           // pixels x - 1
            bf[1][p] = __builtin_bit_cast(f16x8, c);
            bf[2][p] = __builtin_bit_cast(f16x8, u32x4{t01, t12, t23, t3E});           // pixels x + 1
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
// the dy row fragment of output channel j at group gq from the pixel-grouped row image [piece][co][group]
template <class G>
__device__ __forceinline__ void read_dy_frag(const u32x4* sD, int j, int gq, f16x8 (&af)[2]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) af[p] = __builtin_bit_cast(f16x8, sD[(p * 16 + j) * G::NG + gq]);
}

// ---- B. the four K-split partials (waves sp = 0 .. 3 of input-channel block wci) summed through LDS in a fixed order: two rounds,
// two workgroup barriers each.  `red` is [slot][wci][10][4][64] floats over the dead staging image (the row loop ended with a
// barrier); the sum ends in wave sp = 0.  As conv_swrw_body ----
template <int WCI>
__device__ __forceinline__ void ksplit_reduce(float* red, int sp, int wci, int lane, f32x4 (&acc)[9], f32x4& accb) {
#pragma unroll
    for (int s = 2; s >= 1; s >>= 1) {
        if (sp >= s && sp < 2 * s) {
            float* p = red + (size_t)((sp - s) * WCI + wci) * 10 * 256 + lane;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) p[(t * 4 + r) * 64] = acc[t][r];
#pragma unroll
            for (int r = 0; r < 4; ++r) p[(36 + r) * 64] = accb[r];
        }
        __syncthreads();
        if (sp < s) {
            const float* p = red + (size_t)(sp * WCI + wci) * 10 * 256 + lane;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][r] += p[(t * 4 + r) * 64];
#pragma unroll
            for (int r = 0; r < 4; ++r) accb[r] += p[(36 + r) * 64];
        }
        __syncthreads();
    }
}

// ---- C. slab and bias-slab store of wave sp = 0.  Lane (j, kq), register r: co = kq * 4 + r, ci = ci0 + j; the slab is
// [tap][CoutS][CinS] (it may be narrower than the 16 x 16 fragment: the exact-N plan of the class convolution), the bias slab [CoutS].
// PIN: the bias scale in a vector register of its own -- from the scalar pair (scale, 1 / scale) the packed multiply took 1 / scale by
// a low-half op_sel, which tools/isa_lint.py keeps out of the library.  conv_hrwrw_body's epilogue ----
template <bool PIN = false>
__device__ __forceinline__ void store_slabs(float* slab, float* bslab, bool bias, int split, int CoutS, int CinS, int ci0, int j, int kq,
                                            const f32x4 (&acc)[9], const f32x4& accb, float inv_d, float inv_x, unsigned* err) {
    slab += (size_t)split * 9 * CoutS * CinS;
    float chk = 0.f;
    const float inv = inv_d * inv_x;                       // exact: powers of two
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        note_nonfinite(chk, acc[t]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = kq * 4 + r, ci = ci0 + j;
            if (co < CoutS && ci < CinS) slab[((size_t)t * CoutS + co) * CinS + ci] = acc[t][r] * inv;
        }
    }
    report_nonfinite(err, chk, UAPS_ERR_WRW_NONFINITE);
    if (bias && j == 0) {
        float inv_b = inv_d;
        if constexpr (PIN) asm volatile("" : "+v"(inv_b));
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (kq * 4 + r < CoutS) bslab[(size_t)split * CoutS + kq * 4 + r] = accb[r] * inv_b;
    }
}

// ---- D / H state: the per-run coefficients of a staging wave's four channels and the BatchNorm-backward sums of its rows ----
template <class G>
struct BnRowSums {
    f32x2 cf[G::NXL];                                     // (scale, shift) of the activation in front
    float mu[G::NXL], is[G::NXL], sc[G::NXL], sh[G::NXL];    // mean, invstd, gamma invstd, beta
    float st_s[G::NXL][4], st_q[G::NXL][4];               // [channel][row % 4]: the four waves of bn_bwd_sums_max_kernel's block
};

// ---- D. an activated row into the image [piece][ci][slot][group]: leaky_relu(fma(y, scale, shift)) (zero outside the image), scaled
// and split into two fp16 pieces, 8 bytes per lane and piece.  conv_hrwrw_body<1, XF = true>'s store_x ----
template <class G>
__device__ __forceinline__ void store_act_rows(u32x4* sX, f32x4 (&src)[G::NXL], const f32x2 (&cf)[G::NXL], bool ok, float slope, float sc_x,
                                               int xc0, int lane, int slot) {
#pragma unroll
    for (int i = 0; i < G::NXL; ++i) {
        asm volatile("" : "+v"(src[i]));
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float z = __builtin_fmaf(src[i][k], cf[i].x, cf[i].y);
            v[k] = ok ? __builtin_fmaxf(z, z * slope) : 0.f;
        }
        unsigned a0, a1, b0, b1;
        conv_split2h(v[0] * sc_x, v[1] * sc_x, a0, a1);
        conv_split2h(v[2] * sc_x, v[3] * sc_x, b0, b1);
        const int c = xc0 + i;
        unsigned* p0 = reinterpret_cast<unsigned*>(&sX[(c * G::NSLOT + slot) * G::XG + 1]) + lane * 2;
        unsigned* p1 = reinterpret_cast<unsigned*>(&sX[((G::CI + c) * G::NSLOT + slot) * G::XG + 1]) + lane * 2;
        *reinterpret_cast<uint2*>(p0) = make_uint2(a0, b0);
        *reinterpret_cast<uint2*>(p1) = make_uint2(a1, b1);
    }
}

// ---- E. a dy row v[channel][pixel] of a staging wave into slot `slot` of the ring [piece][channel group][slot][column]: the wave's
// four channels (half ch of channel group cg) are two dwords of every pixel's 16-byte unit, for both pieces.  conv_hr16_body's image ----
template <class G>
__device__ __forceinline__ void store_ring_rows(u32x4* sIn, const f32x4 (&v)[4], float scale, int cg, int ch, int lane, int slot) {
    const int base = (cg * G::NSLOT + slot) * G::IW + 4 + lane * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned q00, q01, q10, q11;
        conv_split2h(v[0][k] * scale, v[1][k] * scale, q00, q01);
        conv_split2h(v[2][k] * scale, v[3][k] * scale, q10, q11);
        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned*>(&sIn[base + k]) + ch * 2) = make_uint2(q00, q10);
        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned*>(&sIn[G::PIECE + base + k]) + ch * 2) = make_uint2(q01, q11);
    }
}

// ---- F. input-gradient weight fragments of one wave, loaded once: lane (n = j, k-group kq) of step s holds k-group q = 4 s + kq =
// (tap q / 2, channel group q % 2) of output channel `co` of CoutP packed ones; the wave's tiles are tile0 .. tile0 + MW - 1.
// conv_hr16_body<2>'s fragments and ring offsets ----
template <class G>
struct GradFrags {
    u32x4 bfr[G::NSTEP][2];
    int kxo[G::NSTEP], kyv[G::NSTEP], abase[G::MW];
};
template <class G, int CoutP>
__device__ __forceinline__ void load_grad_frags(GradFrags<G>& f, const float* wp, int CGP, int co, int j, int kq, int tile0) {
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(wp, (uint32_t)(2 * 9) * CGP * CoutP * 16u);
#pragma unroll
    for (int s = 0; s < G::NSTEP; ++s) {
        const int q = 4 * s + kq, tap = q / 2, cgq = q % 2;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const uint32_t off = q < G::NQ ? (uint32_t)(((p * 9 + tap) * CGP + cgq) * CoutP + co) * 16u : kOob;
            f.bfr[s][p] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (int)off, 0, 0);
        }
        const int qq = q < G::NQ ? q : 0;                 // padded k-groups meet zero weights
        f.kxo[s] = (qq % 2) * G::CGU + (qq / 2) % 3; f.kyv[s] = (qq / 2) / 3;
    }
#pragma unroll
    for (int m = 0; m < G::MW; ++m) f.abase[m] = (tile0 + m) * 16 + j + G::XS;
}

// ---- G. one output row of the wave's four 16-pixel tiles from the ring rows in slots s0, s1, s2, added to gacc: conv_hr16_body<2,
// false>'s k order (tap, channel group) and three-product order; the unit loop is software-pipelined (a unit's ring reads are issued
// in front of the previous unit's matrix instructions) ----
template <class G>
__device__ __forceinline__ void grad_row_tiles(const u32x4* sIn, const GradFrags<G>& f, int s0, int s1, int s2, f32x4 (&gacc)[G::MW]) {
    constexpr int NSTEP = G::NSTEP, MW = G::MW;
    int aoff[NSTEP];
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) aoff[s] = f.kxo[s] + (f.kyv[s] == 0 ? s0 : (f.kyv[s] == 1 ? s1 : s2)) * G::IW;
    constexpr int NUN = NSTEP * MW;
    u32x4 af[2][2];
    auto read_a = [&](int u, u32x4 (&dst)[2]) {
        const int s = u / MW, m = u % MW;
#pragma unroll
        for (int p = 0; p < 2; ++p) dst[p] = sIn[p * G::PIECE + f.abase[m] + aoff[s]];
    };
    read_a(0, af[0]);
#pragma unroll
    for (int u = 0; u < NUN; ++u) {
        const int s = u / MW, m = u % MW;
        if (u + 1 < NUN) read_a(u + 1, af[(u + 1) & 1]);
        const auto Hf = [](const u32x4& v) { return __builtin_bit_cast(f16x8, v); };
        f32x4 c = gacc[m];
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Hf(af[u & 1][1]), Hf(f.bfr[s][0]), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Hf(af[u & 1][0]), Hf(f.bfr[s][1]), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Hf(af[u & 1][0]), Hf(f.bfr[s][0]), c, 0, 0, 0);
        gacc[m] = c;
        if (u + 1 < NUN) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      // next unit's DS reads first ...
        __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                       // ... then this unit's MFMAs
    }
}
// the row scaled as conv_hr16_body scales it, checked, and stored into the exchange row [channel][column]: lane (j, kq) holds pixels
// kq * 4 .. kq * 4 + 3 of channel j of every tile
template <class G>
__device__ __forceinline__ void put_grad_row(float* sG, const f32x4 (&gacc)[G::MW], float out_scale_a, float out_scale_w, int j, int kq,
                                             int tile0, unsigned* err) {
    float chk = 0.f;
#pragma unroll
    for (int m = 0; m < G::MW; ++m) {
        f32x4 v = gacc[m];
        v *= out_scale_a; v *= out_scale_w;               // exact: powers of two
        v += 0.f;                                         // (the row kernel adds its absent bias)
        note_nonfinite(chk, v);
        *reinterpret_cast<f32x4*>(&sG[j * G::GS + (tile0 + m) * 16 + kq * 4]) = v;
    }
    report_nonfinite(err, chk, UAPS_ERR_CONV_NONFINITE);
}
// channel c of the exchange row in the staging layout (lane = 4 consecutive pixels), on its way to row t of the output tensor behind
// rs_g: whole 1-KiB rows
template <class G>
__device__ __forceinline__ f32x4 take_row_out(const float* sG, __amdgpu_buffer_rsrc_t rs_g, int c, int t, int HW, int lane) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(&sG[c * G::GS + lane * 4]);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, gv), rs_g, (int)((uint32_t)(c * HW + t * G::WIDTH + lane * 4) * 4u), 0, 0);
    return gv;
}

// ---- H. the BatchNorm-backward sums of a run, bn_bwd_sums_max_kernel's (norm_act.hip) arithmetic and order: a run IS that kernel's
// 4096-float chunk, whose thread (wave v, lane) sums rows v, v + 4, v + 8, v + 12 at this lane's four columns ----
template <class G>
__device__ __forceinline__ void bn_run_begin(BnRowSums<G>& s, const float2* xf, const float* mean, const float* invstd, const float* gamma,
                                             const float* beta, int grp, int xc0) {
#pragma unroll
    for (int i = 0; i < G::NXL; ++i) {
        const int c = xc0 + i;
        const float2 t = xf[(size_t)grp * G::CI + c];
        s.cf[i] = f32x2{t.x, t.y};
        s.mu[i] = mean[grp * G::CI + c]; s.is[i] = invstd[grp * G::CI + c];
        s.sc[i] = gamma[c] * s.is[i]; s.sh[i] = beta[c];
#pragma unroll
        for (int v = 0; v < 4; ++v) { s.st_s[i][v] = 0.f; s.st_q[i][v] = 0.f; }
    }
}
// row t of channel i: gradient gv, raw conv output yv (norm_act.hip's dpre per element); slot 0 of the rotating set is row t's wave
template <class G>
__device__ __forceinline__ void bn_row(BnRowSums<G>& s, int i, const f32x4& gv, const f32x4& yv, float slope, float& md, float& mx) {
    float cs = s.st_s[i][0], cq = s.st_q[i][0];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float yc = yv[e] - s.mu[i], z = yc * s.sc[i] + s.sh[i];
        const float d = z > 0.f ? gv[e] : gv[e] * slope, xh = yc * s.is[i];
        cs += d; cq += d * xh;
        md = __builtin_fmaxf(md, __builtin_fabsf(d)); mx = __builtin_fmaxf(mx, __builtin_fabsf(xh));
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) { s.st_s[i][v] = s.st_s[i][v + 1]; s.st_q[i][v] = s.st_q[i][v + 1]; }
    s.st_s[i][3] = cs; s.st_q[i][3] = cq;
}
// one part per (channel, run) in block_sum2's order: the lane butterfly of each of the four waves, then the waves in turn -- the part
// bn_bwd_sums_max_kernel writes for this chunk.  `partials` is [16][B][rpi]; ri is the run's index inside image b
template <class G>
__device__ __forceinline__ void bn_run_end(const BnRowSums<G>& st, float2* partials, int B, int b, int rpi, int ri, int xc0, int lane) {
#pragma unroll
    for (int i = 0; i < G::NXL; ++i) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float sv = st.st_s[i][v], qv = st.st_q[i][v];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { sv += __shfl_xor(sv, o, 64); qv += __shfl_xor(qv, o, 64); }
            s = v == 0 ? sv : s + sv; q = v == 0 ? qv : q + qv;
        }
        if (lane == 0) partials[((size_t)(xc0 + i) * B + b) * rpi + ri] = make_float2(s, q);
    }
}

// ---- host side of the entry points ----
// whole rounds of the eight XCDs (xcd_swizzle); the workgroups behind nsplit return at once
inline unsigned row_grid(int nsplit) { return (unsigned)((nsplit + 7) / 8 * 8); }

// The slabs of the layer's weight-gradient plan ([split][tap][CoutS][16] + [split][CoutS]: workspace and reduction are the plan's) and
// the BatchNorm-backward operands into the argument struct of a pass that forms both
template <class Args>
inline int row_wrw_bn_args(Args& a, int CoutS, int B, int Cin, int Cout, int H, int W, int ks, int cfg, int want_bias, void* ws, size_t ws_bytes,
                           const float* dy_bound, float dy_mul, const float* x_bound, float x_mul, const float* save_mean,
                           const float* save_invstd, const float* gamma, const float* beta, void* partials, float* maxes) {
    size_t need = 0;
    const int rc = uaps_conv_wrw_workspace_bytes(B, Cin, Cout, H, W, ks, cfg, &need);
    if (rc) return rc;
    constexpr int CinS = 16;
    const size_t per_split = ((size_t)9 * CoutS * CinS + CoutS) * sizeof(float);
    if (need == 0 || need % per_split) return UAPS_ENOFORM;
    if (ws_bytes < need) return UAPS_EWORKSPACE;
    a.nsplit = (int)(need / per_split);
    a.slab = (float*)ws;
    a.bslab = want_bias ? a.slab + (size_t)a.nsplit * 9 * CoutS * CinS : nullptr;
    a.dy_bound = dy_bound; a.dy_mul = dy_mul; a.in_bound = x_bound; a.in_mul = x_mul;
    a.bs_mean = save_mean; a.bs_invstd = save_invstd; a.bs_gamma = gamma; a.bs_beta = beta;
    a.partials = (float2*)partials; a.bs_max = maxes;
    a.err = error_word();
    return UAPS_OK;
}

}  // namespace uaps
