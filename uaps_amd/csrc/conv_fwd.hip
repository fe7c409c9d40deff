// extern "C" entry points of the forward / input-gradient convolution and the weight packing
// (include/uaps_hip.h, section "Convolutions").
#include "../../include/uaps_hip.h"
#include <stdio.h>
#include <stdlib.h>
#include "conv_kernels.hpp"
#include "conv_split.hpp"
#include "conv_split_n16.hpp"
#include "conv_split_row16.hpp"
#include "conv_small.hpp"
#include "conv_gemm1x1.hpp"
#include "conv_split_g.hpp"
#include "hints.hpp"
#include "conv_call.hpp"
using namespace uaps;

// 0 = exact fp32 matrix instructions (v_mfma_f32_16x16x4_f32), 1 = exact 3-way bf16 split on the bf16 matrix pipe,
// 2 (default) = 1, and the two-piece fp16 split for operands with a known magnitude bound (conv_split.hpp).
// Set with uaps_conv_set_mode (the Python layer forwards UAPS_CONV_MODE once at load); the library itself reads no environment.
static int g_conv_mode = 2;
static unsigned g_conv_tuning = 0;      // UAPS_TUNE_* bits (uaps_conv_set_tuning): ablation / diagnosis switches of the planners
static int conv_mode() { return g_conv_mode; }
extern "C" int uaps_conv_set_mode(int mode) {
    if (mode != 0 && mode != 1 && mode != 2) return UAPS_EINVAL;
    g_conv_mode = mode;
    return UAPS_OK;
}
extern "C" int uaps_conv_get_mode(void) { return conv_mode(); }
extern "C" int uaps_conv_set_tuning(unsigned flags) { g_conv_tuning = flags; return UAPS_OK; }
extern "C" unsigned uaps_conv_get_tuning(void) { return g_conv_tuning; }

namespace {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int kdim_pad(int c, int ks) { return (ks == 3 && c <= 4) ? 4 : round_up(c, 8); }   // K (contraction) channels: chunk of 4 or 8
inline int ndim_pad(int c) { return round_up(c, 16); }              // N (output) channels: 16-wide MFMA tiles


// split: one of the bf16-split kernels runs; s32: the 32x32x16 form (3x3, 8x32 tiles, >= 32 output channels)
// small: 1 = the exact-N VALU kernel for <= 4 output channels (conv_small.hpp)
// g1: the GEMM-tiled 1x1 kernels of conv_gemm1x1.hpp (128 consecutive pixels x 128 / 64 output channels per workgroup)
// s32t: 16-row tiles for the 32-channel blocks (the statistics parts stay per 8 rows)
struct FwdPlan { int ck, bn, th, tw; bool vec; int CinP, CoutP, extra_lds, dil; bool split, s32; int sck, sbn; int small; bool g1, s32t;
                 bool bounded, g128; };

int plan_fwd(const void* x, const void* y, int B, int Cin, int Cout, int H, int W, int ks, int cfg, FwdPlan* p) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    if (ks != 1 && ks != 3) return UAPS_ERANGE;
    if ((double)Cin * H * W * 4.0 >= 2147483648.0 || (double)Cout * H * W * 4.0 >= 2147483648.0) return UAPS_ERANGE;
    p->bounded = (cfg & UAPS_CONV_BOUNDED) != 0;      // the caller's promise of operand bounds (include/uaps_hip.h); not a planner setting
    cfg &= ~UAPS_CONV_BOUNDED;
    p->CinP = kdim_pad(Cin, ks); p->CoutP = ndim_pad(Cout);
    p->ck = (ks == 3 && Cin <= 4 && ((cfg >> 24) & 0xf) <= 1) ? 4 : 8;
    // 16-byte loads/stores need rows that start 16-byte aligned
    p->vec = (W % 4 == 0) && ((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0);
    // pixel tile: 8 rows x 32 columns, or 16 x 16 for narrow maps (both 256 pixels = 16 M tiles)
    const bool wide = ((cfg >> 24) & 0xf) > 1 ? true : (((cfg >> 8) & 3) ? (((cfg >> 8) & 3) == 1) : (W >= 32));
    p->extra_lds = ((cfg >> 16) & 0xff) * 1024;
    p->dil = ((cfg >> 24) & 0xf) ? ((cfg >> 24) & 0xf) : 1;
    if (p->dil != 1 && (ks != 3 || (p->dil != 2 && p->dil != 4) || Cin <= 4)) return UAPS_ERANGE;
    p->th = wide ? 8 : 16; p->tw = wide ? 32 : 16;
    int bn = (p->CoutP % 64 == 0) ? 64 : (p->CoutP % 32 == 0 ? 32 : 16);
    const long tiles = (long)B * ((H + p->th - 1) / p->th) * ((W + p->tw - 1) / p->tw);
    while (bn > 16 && tiles * (p->CoutP / bn) < 512) bn /= 2;       // at least two workgroups per CU
    if (cfg & 0xff) { bn = cfg & 0xff; if ((bn != 16 && bn != 32 && bn != 64) || p->CoutP % bn) return UAPS_EINVAL; }
    if (p->ck == 4) bn = 16;
    p->bn = bn;
    p->small = 0;
    if (ks == 3 && p->dil == 1 && W % 4 == 0 && W >= 64 && H >= 8 && !(cfg & 0x70ffffff)) {
        if (Cout <= 4 && Cin % 8 == 0 && Cin <= 32) p->small = 1;      // conv_small_body: KMAX
        // (the mirror case, <= 4 contraction channels -> 16 outputs, measured 52 us against 47 us of the fp32 MFMA kernel at
        // 4 -> 16 @ 256 x 256, B = 32: not used)
    }
    // the split-bf16 form: 16-byte rows, no dilation, no forced tile / LDS settings; cfg bit 28 forces the exact kernels
    // cfg bits 29-30 select among them for tools/bench_modes.py: 1 = the 16x16x32 form, 2 = the 32x32x16 form (low byte: BN)
    // measured (tools/bench_modes.py, B = 32): the split forms win 1.2-1.7x on every 3x3 layer with more than 8 contraction
    // channels and lose on 1x1 convolutions (HBM-bound, the split only adds staging work) and on the <= 8-channel layers
    // (a chunk of 8 channels fills 9 of 12 k-groups); cfg bits 29-30 != 0 force a split form regardless
    // 1x1 convolutions: narrow ones, and wide ones on maps of fewer than 32 x 32 pixels (the U-Net's 256 -> 128 projection at a
    // 256^2 input), are HBM- or launch-bound and stay on the fp32 instruction; from 1024 pixels on (the same projection at a 512^2
    // input, and the bottleneck projections of the ResNet encoders: 64 ... 2048 channels, utilities/resnet.py:55-95) they are
    // compute-bound and take the split form.  plan_wrw (conv_wrw.hip) applies the same rule.
    const bool big_1x1 = ks == 1 && Cin >= 64 && (long)Cin * Cout >= 16384 && (long)H * W >= 1024;
    // dilated 3x3 (ResNet stages): the 32x32x16 split form only (>= 32 output channels, no forced settings)
    const bool dil_ok = p->dil == 1 || (ks == 3 && Cin > 8 && p->CoutP % 32 == 0 && !(cfg & 0x70ffffff));
    p->split = conv_mode() >= 1 && dil_ok && (W % 4 == 0) && !(cfg & 0x10ffff00) && ((ks == 3 && Cin > 8) || big_1x1 || ((cfg >> 29) & 3));
    if (g_conv_tuning & UAPS_TUNE_NO_SPLIT_FWD) p->split = false;
    p->g1 = p->split && big_1x1 && p->vec && p->CoutP % 64 == 0 && !(cfg & 0x7fffffff);
    const int sel = (cfg >> 29) & 3, bn_req = cfg & 0xff;
    p->sck = ks == 1 ? 32 : (Cin <= 8 ? 8 : 16);
    // 32 output channels per workgroup from 256 workgroups on (round 5, profiles/r05_mfma_shape_ab.txt: 256 -> 256 @ 16 x 16, B = 32:
    // 42.4 against 46.1 us with 16, 128 -> 256: 23.6 against 25.3; with 128 workgroups -- 256 -> 128 -- 16 stays faster, 34.0 against 40.4)
    p->sbn = (p->CoutP % 32 == 0 && tiles * (p->CoutP / 32) >= 256) ? 32 : 16;
    p->s32 = p->split && ks == 3 && p->tw == 32 && p->CoutP % 32 == 0 && sel != 1;
    // round 5 (profiles/r05_mfma_shape_ab.txt, same per-wave tile of 64 pixels x 32 channels): on maps of <= 32 x 32 pixels with >= 128
    // contraction channels and 128 output channels the 16x16x32 form with 16-channel chunks is 3-5 % faster than either 32x32x16 form
    // (128 -> 128: 33.1 against 34.3 us, 256 -> 128: 59.2 against 62.4 us at B = 32); everywhere else it loses 4-15 %
    // (measured in the fp16-split arithmetic only: mode 2)
    if (p->s32 && conv_mode() == 2 && sel == 0 && !bn_req && p->dil == 1 && (long)H * W <= 1024 && Cin >= 128 && p->CoutP == 128 &&
        tiles * (p->CoutP / 32) >= 512) { p->s32 = false; p->sbn = 32; p->sck = 16; }
    if (p->s32) {
        p->sck = 8;
        p->sbn = (p->CoutP % 64 == 0 && tiles * (p->CoutP / 64) >= 512) ? 64 : 32;
        if (bn_req == 32 || (bn_req == 64 && p->CoutP % 64 == 0)) p->sbn = bn_req;
        // 32-channel blocks: 16-row tiles while that still gives every CU two workgroups (UAPS_TUNE_NO_TALL_FWD keeps the 8-row tiles)
        const long tiles16 = (long)B * ((H + 15) / 16) * ((W + 31) / 32);
        p->s32t = p->sbn == 32 && p->dil == 1 && !(g_conv_tuning & UAPS_TUNE_NO_TALL_FWD) &&
                  tiles16 * (p->CoutP / 32) >= 512;
    } else if (p->split && bn_req) {
        if ((bn_req != 16 && bn_req != 32) || p->CoutP % bn_req) return UAPS_EINVAL;
        p->sbn = bn_req;
    }
    // round 6 (csrc/conv_split_g.hpp): 128-output-channel layers on 32-wide maps as ONE workgroup per 4-row band and 128 channels --
    // every input element staged once per layer, 32-channel chunks, weight fragments straight from L2; fp16-split arithmetic only
    // (exactly 128 output channels: with 256 -- the input gradient of up1's first convolution -- the form needs two rounds of one
    // workgroup per CU and stages the input twice: 100 us against 63.5 us of conv_h32_kernel<64>, profiles/r06_hg128_ab.txt)
    p->g128 = p->split && conv_mode() == 2 && ks == 3 && p->dil == 1 && W == 32 && H % 4 == 0 && Cin % 32 == 0 && Cout == 128 && p->vec &&
              !(cfg & 0x7fffffff) && !(g_conv_tuning & UAPS_TUNE_NO_G);
    return UAPS_OK;
}

// uaps_conv_fwd_stats_parts: the BatchNorm-partials layout that shape and cfg alone decide -- one part per pixel tile of the plan, per
// 128 pixels of the GEMM-tiled plan, or (UAPS_CONV_BOUNDED) per 4-row band of the whole-layer-width plan (conv_split_g.hpp)
int stats_parts(int B, int Cin, int Cout, int H, int W, int ks, int cfg, int* parts) {
    FwdPlan p{};
    const int rc = plan_fwd(nullptr, nullptr, B, Cin, Cout, H, W, ks, cfg, &p);
    if (rc) return rc;
    *parts = (p.g128 && p.bounded) ? H / 4 : p.g1 ? (H * W + 127) / 128 : ((H + p.th - 1) / p.th) * ((W + p.tw - 1) / p.tw);
    return UAPS_OK;
}

// The kernel forms of the forward / input gradient (each a family of conv_*_kernel instantiations; the split forms come as 's' = three
// bf16 pieces and 'h' = two fp16 pieces, most also with the staging-time BatchNorm of xf: `_bn`)
enum class FwdKind {
    Tile,      // conv_fwd_kernel<ks, th, tw, n, ck, vec, dil>: the fp32 matrix instruction
    Small,     // conv_small_kernel<8, 4>: the exact-N VALU kernel (<= 4 output channels)
    Split,     // conv_sfwd / conv_hfwd_kernel<ks, th, tw, n, ck>
    S32,       // conv_s32 / conv_h32_kernel<n>: the 32x32x16 form, 8 x 32 tiles
    S32T,      // conv_s32t / conv_h32t_kernel<32>: 16-row tiles
    S32D,      // conv_s32d / conv_h32d_kernel<n, dil>: dilated
    G1,        // conv_g1s_kernel<n>, conv_g1h_kernel<n>, conv_g1h256_kernel: GEMM-tiled 1x1
    HG128,     // conv_hg128_kernel (conv_hg128_deep_kernel): one workgroup per 4-row band x 128 channels
    HP16,      // conv_hp16_kernel<n>: persistent, 16 output channels
    HR16,      // conv_hr16_kernel<n> (conv_hr16w_kernel: 256-wide column strips): full-width rows, 16 output channels
    HR16Up,    // conv_hr16_up_kernel: x2 up-sampled while staged (UAPS_CONV_X2_UP2)
    HR16Bs,    // conv_hr16_bs_kernel: BatchNorm-backward sums in the epilogue (uaps_call_hints::bsum_*)
    HR16x2,    // conv_hr16x2_kernel (conv_hr16wx2_kernel): 16 -> 32 channels as two output tiles
};

// What one call runs: the kernel with its template parameters, the launch geometry and the BatchNorm-partials layout it writes
struct FwdForm {
    FwdPlan plan;
    FwdKind kind;
    int ks, th, tw, n, ck, dil;        // template parameters (n: output channels per workgroup; HP16 / HR16: 2 or 4)
    bool vec, h16, bn, deep, strips;   // 16-byte rows; fp16 pieces; staging-time BatchNorm; HG128 deep; HR16 column strips
    bool up2;
    int Csplit, Osplit;                // the concatenation splits (Cin / Cout: one tensor)
    unsigned grid, block; int lds;
    int tiles_x, tiles_y, nblk;
    int parts;                         // BatchNorm partials per image
};

bool split_form(FwdKind k) { return k != FwdKind::Tile && k != FwdKind::Small; }
unsigned grid8(long n) { return (unsigned)((n + 7) / 8 * 8); }      // a multiple of 8 for the XCD swizzle

// Which kernel the call runs.  Every condition of that choice is here, host code only (no HIP call): a query needs no GPU.  The
// optional requests (up2, bsum, out_amax, stats) that only some forms honour are checked against the result by check_fwd.
int resolve_fwd(const uaps_call_hints& h, const FwdCall& c, FwdForm* out) {
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, H = c.H, W = c.W, ks = c.ks;
    const void* xf = c.xf;
    // UAPS_CONV_X2_UP2: x2 is [B, Cin - Csplit, H / 2, W / 2] and is up-sampled x2 (bilinear, align_corners) while staged
    const bool up2 = (c.cfg & UAPS_CONV_X2_UP2) != 0;
    const int cfg = c.cfg & ~UAPS_CONV_X2_UP2;
    if (up2 && (!c.x2 || H % 2 || W % 2)) return UAPS_EINVAL;
    if (xf && (c.x2 || c.groups < 1 || B % c.groups || (uintptr_t)xf % 8)) return UAPS_EINVAL;
    if (xf && !(c.xf_slope >= 0.f && c.xf_slope <= 1.f)) return UAPS_ERANGE;      // leaky_relu is evaluated as max(z, slope * z)
    const int Csplit = (c.Csplit < 0 || !c.x2) ? Cin : c.Csplit;
    const int Osplit = (c.Osplit < 0 || !c.y2) ? Cout : c.Osplit;
    if (Csplit > Cin || Osplit > Cout || (Csplit < Cin && (Csplit % 8 || Csplit == 0)) || (Osplit < Cout && Osplit == 0)) return UAPS_EINVAL;
    FwdForm f{};
    FwdPlan& p = f.plan;
    const int rc = plan_fwd(c.x, c.y, B, Cin, Cout, H, W, ks, cfg, &p);
    if (rc) return rc;
    if ((c.x2 && !up2 && (uintptr_t)c.x2 % 16) || (c.y2 && (uintptr_t)c.y2 % 16)) p.vec = false;
    if (!p.vec || (Csplit < Cin && Csplit % p.sck)) p.split = false;      // unaligned tensors / odd concat split: exact kernels
    if (p.dil > 1 && (!p.s32 || c.x2 || c.y2 || xf)) p.split = false;    // the dilated split form: one tensor per side, no staging BatchNorm
    const bool bsum = h.bsum_y != nullptr;
    if (bsum && (!h.bsum_mean || !h.bsum_invstd || !h.bsum_gamma || !h.bsum_beta || !h.bsum_partials || !h.bsum_max || h.bsum_groups < 1 ||
                 B % h.bsum_groups || !(h.bsum_slope >= 0.f && h.bsum_slope <= 1.f)))
        return UAPS_EINVAL;
    f.ks = ks; f.th = p.th; f.tw = p.tw; f.n = p.bn; f.ck = p.ck; f.dil = p.dil; f.vec = p.vec; f.bn = xf != nullptr;
    f.up2 = up2; f.Csplit = Csplit; f.Osplit = Osplit;
    f.parts = ((H + p.th - 1) / p.th) * ((W + p.tw - 1) / p.tw);      // one part per tile of the plan (s32t too: per 8 rows)
    const unsigned tune = g_conv_tuning;
    const bool wide = p.tw == 32;
    // (on 256-wide maps with bounded operands the full-width-row kernel serves <= 4 output channels too: padded to one 16-channel
    // MFMA tile it streams at the HBM rate of a 16 -> 16 layer, which the 16 x 64-tile VALU kernel does not reach)
    const bool row16 = p.split && conv_mode() == 2 && h.bound[0] && ks == 3 && p.dil == 1 && W % 256 == 0 && H % 16 == 0 && p.CoutP == 16 &&
                       Cin > 8 && Cin <= 32 && Cin % 8 == 0 && !c.y2 && (!c.x2 || Csplit >= Cin || h.bound[1]) &&
                       !(tune & (UAPS_TUNE_NO_ROW16 | UAPS_TUNE_NO_HP16));
    // a side with <= 4 channels: the exact-N fp32 kernels (no BatchNorm statistics epilogue, one tensor per side)
    if (!(tune & UAPS_TUNE_NO_SMALL) && !row16 && p.small && p.vec && !c.stats && !c.x2 && !c.y2 && (p.small == 1 || !xf)) {
        f.kind = FwdKind::Small;
    } else if (p.split) {
        // mode 2 and every tensor operand bounded: the two-piece fp16 form
        f.h16 = conv_mode() == 2 && h.bound[0] && (!c.x2 || Csplit >= Cin || h.bound[1]);
        f.n = p.sbn;
        // the whole-layer-width tile form (conv_split_g.hpp): with statistics only when the caller promised the bounds up front
        // (UAPS_CONV_BOUNDED: the partial-sum layout of this form is what uaps_conv_fwd_stats_parts reported for the same bit)
        // (not with the staging-time BatchNorm: its transform sits exposed in a one-wave-per-SIMD kernel -- 46.7 against 41.1 us of
        // conv_hfwd_bn_kernel -- so such calls keep the tile kernels AND their partial-sum layout: see uaps_conv_fwd_stats_parts)
        if (p.g128 && !xf && f.h16 && (!c.stats || p.bounded) && (Csplit == Cin || Csplit % 32 == 0) && (Osplit == Cout || Osplit % 128 == 0) &&
            !h.out_amax && !bsum && !up2) {
            f.kind = FwdKind::HG128;
            f.deep = (tune & UAPS_TUNE_G_DEEP) != 0;
            f.parts = H / 4;
        } else if (p.g1 && !c.x2 && !c.y2 && !xf) {
            // (no two-tensor / BatchNorm-in-staging form of the GEMM-tiled kernels: those take the 3x3-style tiling)
            f.kind = FwdKind::G1;
            f.parts = (H * W + 127) / 128;
            f.n = (f.h16 && p.CoutP % 256 == 0 && !(tune & UAPS_TUNE_G1_NARROW)) ? 256 : (p.CoutP % 128 == 0 ? 128 : 64);
        } else if (f.h16 && ks == 3 && p.dil == 1 && Cin == 16 && Cout == 32 && !c.stats && !xf && !c.x2 && (Osplit == Cout || Osplit == 16) &&
                   W % 256 == 0 && H % 16 == 0 && !(tune & (UAPS_TUNE_NO_ROW16 | UAPS_TUNE_NO_HP16))) {
            // 16 -> 32 channels on a 256-wide map without statistics (the input gradient of up4's two-tensor convolution): two output
            // tiles of the full-width-row kernel, written as one or two 16-channel tensors
            f.kind = FwdKind::HR16x2;
            f.strips = W > 256;
        } else if (p.dil > 1) {
            f.kind = FwdKind::S32D;
        } else if (p.s32) {
            f.kind = p.s32t ? FwdKind::S32T : FwdKind::S32;
        } else if (!(tune & UAPS_TUNE_NO_HP16) && f.h16 && ks == 3 && wide && p.CoutP == 16 && Cin > 8 && Cin <= 32 && Osplit == Cout) {
            f.n = Cin <= 16 ? 2 : 4;
            f.strips = W > 256;
            // the up-sampling form exists in ONE kernel: up4's first convolution on a 256-wide map (16 + 16 -> 16 channels)
            if (up2 && row16 && Csplit == 16 && Cin == 32 && W == 256 && up2_pattern_ok(W / 2)) f.kind = FwdKind::HR16Up;
            // BatchNorm-backward sums in the epilogue: ONE kernel, the 16 -> 16 input gradient on a 256-wide map
            else if (bsum && row16 && !c.x2 && !xf && !c.stats && !up2 && Cin == 16 && Cout == 16 && W == 256 &&
                     (uintptr_t)h.bsum_y % 16 == 0 && (uintptr_t)h.bsum_max % 16 == 0) f.kind = FwdKind::HR16Bs;
            else if (W % 256 == 0 && H % 16 == 0 && !(tune & UAPS_TUNE_NO_ROW16)) f.kind = FwdKind::HR16;
            else f.kind = FwdKind::HP16;
        } else {
            f.kind = FwdKind::Split;
            f.n = p.sbn == 16 ? 16 : 32;
            f.ck = ks == 1 ? 32 : (p.sck == 8 ? 8 : 16);
        }
    } else {
        f.kind = FwdKind::Tile;
        // the staging-time BatchNorm: 16-byte form, 8-channel chunks, no dilation
        if (xf && (!p.vec || p.ck != 8 || p.dil != 1)) return UAPS_ERANGE;
    }
    // launch geometry
    long n = 0;
    f.block = kConvThreads;
    switch (f.kind) {
    case FwdKind::Tile: case FwdKind::Split: case FwdKind::S32: case FwdKind::S32T: case FwdKind::S32D:
        if (f.kind == FwdKind::S32 || f.kind == FwdKind::S32D) { f.th = 8; f.tw = 32; }
        if (f.kind == FwdKind::S32T) { f.th = 16; f.tw = 32; f.n = 32; }
        f.tiles_x = (W + f.tw - 1) / f.tw; f.tiles_y = (H + f.th - 1) / f.th; f.nblk = p.CoutP / f.n;
        n = (long)B * f.tiles_x * f.tiles_y * f.nblk;
        if (f.kind == FwdKind::Tile) f.lds = p.extra_lds;     // unused dynamic LDS, requested only to cap the co-resident workgroups per CU
        f.th = p.th; f.tw = p.tw;                             // (the names carry the plan's tile)
        break;
    case FwdKind::G1:
        f.tiles_x = (H * W + 127) / 128; f.tiles_y = 1; f.nblk = p.CoutP / f.n;
        n = (long)B * f.tiles_x * f.nblk;
        break;
    case FwdKind::HG128:
        f.tiles_x = 1; f.tiles_y = H / 4; f.nblk = Cout / 128;
        n = (long)B * f.tiles_y * f.nblk;
        f.block = kHg128Threads; f.lds = kHg128Lds;
        break;
    case FwdKind::Small:
        f.tiles_x = (W + 63) / 64; f.tiles_y = (H + 15) / 16; f.nblk = 1;
        n = (long)B * f.tiles_x * f.tiles_y;
        break;
    case FwdKind::HP16: {
        f.tiles_x = (W + 31) / 32; f.tiles_y = (H + 7) / 8; f.nblk = 1;
        const long ntiles = (long)B * f.tiles_x * f.tiles_y;
        if (ntiles <= 0 || ntiles > 0x7fffffffL) return UAPS_EINVAL;
        // one resident round: 3 (16 input channels) or 2 (32) workgroups fit a CU (registers), 256 CUs; forcing 4 spills and is slower
        const long want = Cin <= 16 ? 768 : 512;
        f.grid = grid8(ntiles < want ? ntiles : want);
        return *out = f, UAPS_OK;
    }
    case FwdKind::HR16: case FwdKind::HR16Up: case FwdKind::HR16Bs: case FwdKind::HR16x2: {
        // runs of 16 rows of one 256-wide column strip; HR16: 2 workgroups of 256 threads per CU for 16 input channels, 1 workgroup of
        // 512 threads (135 KB of LDS) for 32
        const long nruns = (long)B * (H / 16) * (f.kind == FwdKind::HR16 || f.kind == FwdKind::HR16x2 ? W / 256 : 1);
        if (nruns <= 0 || nruns > 0x7fffffffL) return UAPS_EINVAL;
        const long want = f.kind == FwdKind::HR16Up ? 256 : (f.kind == FwdKind::HR16 && Cin > 16) ? 256 : 512;
        f.grid = grid8(nruns < want ? nruns : want);
        f.block = (f.kind == FwdKind::HR16Up || (f.kind == FwdKind::HR16 && Cin > 16)) ? 512 : 256;
        return *out = f, UAPS_OK;
    }
    }
    if (n <= 0 || (n + 7) / 8 * 8 > 0x7fffffffL) return UAPS_EINVAL;
    f.grid = grid8(n);
    *out = f;
    return UAPS_OK;
}

// The call's optional requests against its resolved form (nothing is launched when one fails)
int check_fwd(const uaps_call_hints& h, const FwdCall& c, const FwdForm& f) {
    const FwdPlan& p = f.plan;
    // UAPS_CONV_BOUNDED on a shape of the whole-layer-width form: the caller promised bounds for every operand, and the staging-time
    // BatchNorm has no such form (the bit changes the statistics layout)
    if (split_form(f.kind) && p.g128 && p.bounded && c.stats && (c.xf || !f.h16)) return UAPS_EINVAL;
    // the partials must come in the layout uaps_conv_fwd_stats_parts reported for the shape and cfg (the Python layer hands a call
    // that cannot run the GEMM-tiled plan cfg bit 28: conv.plan_cfg)
    int parts = 0;
    if (c.stats && (stats_parts(c.B, c.Cin, c.Cout, c.H, c.W, c.ks, c.cfg & ~UAPS_CONV_X2_UP2, &parts) || parts != f.parts)) return UAPS_ERANGE;
    // out_amax: raised to max|y| by the fp32-instruction kernels only (the U-Net's 1x1 projections, whose output has no BatchNorm
    // behind it to bound it)
    if (h.out_amax && (f.kind != FwdKind::Tile || p.small || p.g1 || (uintptr_t)h.out_amax % 16)) return UAPS_ENOFORM;
    if (h.bsum_y && f.kind != FwdKind::HR16Bs) return UAPS_ENOFORM;
    if (f.up2 && f.kind != FwdKind::HR16Up) return UAPS_ENOFORM;
    return UAPS_OK;
}

// ---- the launch: a switch on the form (no choice is made below; the form names one instantiation) ----
using FwdKernel = void (*)(ConvFwdArgs);

template <int KS, int TH, int TW, int BN, int CK, int DIL>
FwdKernel tile_kernel(const FwdForm& f) {
    if constexpr (DIL == 1 && CK == 8) {
        if (f.bn) return conv_fwd_bn_kernel<KS, TH, TW, BN, CK, 4, 1>;
    }
    return f.vec ? conv_fwd_kernel<KS, TH, TW, BN, CK, 4, DIL> : conv_fwd_kernel<KS, TH, TW, BN, CK, 1, DIL>;
}
template <int KS, int TH, int TW, int DIL>
FwdKernel tile_kernel_n(const FwdForm& f) {
    if constexpr (KS == 3 && DIL == 1) {
        if (f.ck == 4) return tile_kernel<KS, TH, TW, 16, 4, 1>(f);
    }
    return f.n == 16 ? tile_kernel<KS, TH, TW, 16, 8, DIL>(f) : f.n == 32 ? tile_kernel<KS, TH, TW, 32, 8, DIL>(f) : tile_kernel<KS, TH, TW, 64, 8, DIL>(f);
}

template <int KS, int TH, int TW, int BN, int CK>
FwdKernel split_kernel(const FwdForm& f) {
    if (f.h16) return f.bn ? conv_hfwd_bn_kernel<KS, TH, TW, BN, CK> : conv_hfwd_kernel<KS, TH, TW, BN, CK>;
    return f.bn ? conv_sfwd_bn_kernel<KS, TH, TW, BN, CK> : conv_sfwd_kernel<KS, TH, TW, BN, CK>;
}
template <int KS, int TH, int TW>
FwdKernel split_kernel_n(const FwdForm& f) {
    if constexpr (KS == 3) {
        if (f.ck == 8) return f.n == 16 ? split_kernel<3, TH, TW, 16, 8>(f) : split_kernel<3, TH, TW, 32, 8>(f);
        return f.n == 16 ? split_kernel<3, TH, TW, 16, 16>(f) : split_kernel<3, TH, TW, 32, 16>(f);
    } else {
        return f.n == 16 ? split_kernel<1, TH, TW, 16, 32>(f) : split_kernel<1, TH, TW, 32, 32>(f);
    }
}

template <int BN>
FwdKernel s32_kernel(const FwdForm& f) {
    if (f.h16) return f.bn ? conv_h32_bn_kernel<BN> : conv_h32_kernel<BN>;
    return f.bn ? conv_s32_bn_kernel<BN> : conv_s32_kernel<BN>;
}
template <int BN>
FwdKernel s32d_kernel(const FwdForm& f) {
    if (f.h16) return f.dil == 2 ? conv_h32d_kernel<BN, 2> : conv_h32d_kernel<BN, 4>;
    return f.dil == 2 ? conv_s32d_kernel<BN, 2> : conv_s32d_kernel<BN, 4>;
}
template <int N>
FwdKernel row16_kernel(const FwdForm& f) {
    if (f.kind == FwdKind::HP16) return f.bn ? conv_hp16_bn_kernel<N> : conv_hp16_kernel<N>;
    if (f.strips) return f.bn ? conv_hr16w_bn_kernel<N> : conv_hr16w_kernel<N>;
    return f.bn ? conv_hr16_bn_kernel<N> : conv_hr16_kernel<N>;
}

FwdKernel fwd_kernel(const FwdForm& f) {
    switch (f.kind) {
    case FwdKind::Tile:
        if (f.dil > 1) return f.dil == 2 ? tile_kernel_n<3, 8, 32, 2>(f) : tile_kernel_n<3, 8, 32, 4>(f);
        if (f.ks == 3) return f.tw == 32 ? tile_kernel_n<3, 8, 32, 1>(f) : tile_kernel_n<3, 16, 16, 1>(f);
        return f.tw == 32 ? tile_kernel_n<1, 8, 32, 1>(f) : tile_kernel_n<1, 16, 16, 1>(f);
    case FwdKind::Small: return f.bn ? conv_small_bn_kernel<8, 4> : conv_small_kernel<8, 4>;
    case FwdKind::Split:
        if (f.ks == 3) return f.tw == 32 ? split_kernel_n<3, 8, 32>(f) : split_kernel_n<3, 16, 16>(f);
        return f.tw == 32 ? split_kernel_n<1, 8, 32>(f) : split_kernel_n<1, 16, 16>(f);
    case FwdKind::S32: return f.n == 64 ? s32_kernel<64>(f) : s32_kernel<32>(f);
    case FwdKind::S32T:
        if (f.h16) return f.bn ? conv_h32t_bn_kernel<32> : conv_h32t_kernel<32>;
        return f.bn ? conv_s32t_bn_kernel<32> : conv_s32t_kernel<32>;
    case FwdKind::S32D: return f.n == 64 ? s32d_kernel<64>(f) : s32d_kernel<32>(f);
    case FwdKind::G1:
        if (!f.h16) return f.n == 128 ? conv_g1s_kernel<128> : conv_g1s_kernel<64>;
        return f.n == 256 ? conv_g1h256_kernel : f.n == 128 ? conv_g1h_kernel<128> : conv_g1h_kernel<64>;
    case FwdKind::HG128: return f.bn ? conv_hg128_bn_kernel : f.deep ? conv_hg128_deep_kernel : conv_hg128_kernel;
    case FwdKind::HP16: case FwdKind::HR16: return f.n == 2 ? row16_kernel<2>(f) : row16_kernel<4>(f);
    case FwdKind::HR16Up: return conv_hr16_up_kernel;
    case FwdKind::HR16Bs: return conv_hr16_bs_kernel;
    case FwdKind::HR16x2: return f.strips ? conv_hr16wx2_kernel : conv_hr16x2_kernel;
    }
    return nullptr;
}

int launch_fwd(const uaps_call_hints& h, const FwdCall& c, const FwdForm& f, hipStream_t s) {
    const FwdPlan& p = f.plan;
    const int ks = c.ks, Cin = c.Cin;
    ConvFwdArgs a{};
    a.in = c.x; a.in2 = c.x2; a.Csplit = f.Csplit; a.out2 = c.y2; a.Osplit = f.Osplit;
    a.wp = c.wp; a.bias = c.bias; a.out = c.y; a.stats = (float2*)c.stats;
    if (c.stats) { a.stats_mean = h.stats_mean; a.stats_bias = h.stats_bias; }
    a.B = c.B; a.Cin = Cin; a.Cout = c.Cout; a.H = c.H; a.W = c.W;
    a.CinP = p.CinP; a.CoutP = p.CoutP;
    a.xf = (const float2*)c.xf; a.xf_slope = c.xf_slope; a.xf_Bg = c.xf ? c.B / c.groups : c.B;
    a.amax = h.out_amax;
    a.tiles_x = f.tiles_x; a.tiles_y = f.tiles_y; a.nblk = f.nblk;
    if (split_form(f.kind)) {
        // the split weights follow the exact ones in the packed buffer (uaps_conv_pack_floats)
        a.wp = c.wp + (size_t)ks * ks * p.CinP * p.CoutP;
        a.CinP = split_cgroups(Cin);
        if (f.h16) {                                  // the fp16 pieces follow the bf16 ones behind a header
            const size_t piece = (size_t)ks * ks * a.CinP * p.CoutP * 4;
            a.wscale = a.wp + 3 * piece + 16;         // {s, 1 / s, max|w|} behind the 16 partial maxima
            a.wp = a.wp + 3 * piece + kH16Header;
            a.in_bound = h.bound[0]; a.in_mul = h.mul[0];
            if (c.x2 && f.Csplit < Cin) { a.in2_bound = h.bound[1]; a.in2_mul = h.mul[1]; }
            a.err = uaps::error_word();
        }
    }
    if (f.kind == FwdKind::HG128) {
        static bool attr = false;
        if (!attr) {                                  // (idempotent; > 48 KB of dynamic LDS needs the attribute once per kernel)
            (void)hipFuncSetAttribute((const void*)conv_hg128_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kHg128Lds);
            (void)hipFuncSetAttribute((const void*)conv_hg128_bn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kHg128Lds);
            (void)hipFuncSetAttribute((const void*)conv_hg128_deep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kHg128Lds);
            attr = true;
        }
    } else if (f.kind == FwdKind::HR16Up) {
        a.up_rh = (float)(c.H / 2 - 1) / (float)(c.H - 1); a.up_rw = (float)(c.W / 2 - 1) / (float)(c.W - 1);      // as uaps_up_cat_fwd
    } else if (f.kind == FwdKind::HR16Bs) {
        a.bs_y = h.bsum_y; a.bs_mean = h.bsum_mean; a.bs_invstd = h.bsum_invstd; a.bs_gamma = h.bsum_gamma;
        a.bs_beta = h.bsum_beta; a.bs_slope = h.bsum_slope; a.bs_Bg = c.B / h.bsum_groups; a.bs_max = h.bsum_max;
        a.stats = (float2*)h.bsum_partials;
        uaps::account_bytes(4.0 * c.B * c.H * c.W * c.Cout);      // the BatchNorm's raw input, once more
    }
    UAPS_LAUNCH_MAIN(fwd_kernel(f), dim3(f.grid), dim3(f.block), f.lds, s, a);
    return (int)hipGetLastError();
}

// the rocprofv3 name of a form's kernel (without namespace)
void fwd_form_name(const FwdForm& f, char* buf, size_t len) {
    const char* bn = f.bn ? "_bn" : "";
    const char hs = f.h16 ? 'h' : 's';
    switch (f.kind) {
    case FwdKind::Tile: snprintf(buf, len, "conv_fwd%s_kernel<%d, %d, %d, %d, %d, %d, %d>", bn, f.ks, f.th, f.tw, f.n, f.ck, f.vec ? 4 : 1, f.dil); break;
    case FwdKind::Small: snprintf(buf, len, "conv_small%s_kernel<8, 4>", bn); break;
    case FwdKind::Split: snprintf(buf, len, "conv_%cfwd%s_kernel<%d, %d, %d, %d, %d>", hs, bn, f.ks, f.th, f.tw, f.n, f.ck); break;
    case FwdKind::S32: snprintf(buf, len, "conv_%c32%s_kernel<%d>", hs, bn, f.n); break;
    case FwdKind::S32T: snprintf(buf, len, "conv_%c32t%s_kernel<32>", hs, bn); break;
    case FwdKind::S32D: snprintf(buf, len, "conv_%c32d_kernel<%d, %d>", hs, f.n, f.dil); break;
    case FwdKind::G1:
        if (f.h16 && f.n == 256) snprintf(buf, len, "conv_g1h256_kernel");
        else snprintf(buf, len, "conv_g1%c_kernel<%d>", hs, f.n);
        break;
    case FwdKind::HG128: snprintf(buf, len, "conv_hg128%s_kernel", f.bn ? "_bn" : f.deep ? "_deep" : ""); break;
    case FwdKind::HP16: snprintf(buf, len, "conv_hp16%s_kernel<%d>", bn, f.n); break;
    case FwdKind::HR16: snprintf(buf, len, "conv_hr16%s%s_kernel<%d>", f.strips ? "w" : "", bn, f.n); break;
    case FwdKind::HR16Up: snprintf(buf, len, "conv_hr16_up_kernel"); break;
    case FwdKind::HR16Bs: snprintf(buf, len, "conv_hr16_bs_kernel"); break;
    case FwdKind::HR16x2: snprintf(buf, len, "conv_hr16%sx2_kernel", f.strips ? "w" : ""); break;
    }
}

}  // namespace

int uaps::conv_fwd_run(const uaps_call_hints& h, const FwdCall& c, uaps_stream_t stream) {
    if (!c.x || !c.wp || !c.y) return UAPS_EINVAL;
    FwdForm f;
    int rc = resolve_fwd(h, c, &f);
    if (rc) return rc;
    // every input and output element once
    uaps::account_bytes(4.0 * c.B * c.H * c.W * ((double)f.Csplit + (c.Cin - f.Csplit) * (f.up2 ? 0.25 : 1.0) + c.Cout));
    rc = check_fwd(h, c, f);
    if (rc) return rc;
    return launch_fwd(h, c, f, (hipStream_t)stream);
}

int uaps::conv_fwd_name(const uaps_call_hints& h, const FwdCall& c, char* buf, size_t buflen) {
    FwdForm f;
    int rc = resolve_fwd(h, c, &f);
    if (!rc) rc = check_fwd(h, c, f);
    if (rc) return rc;
    if (!buf || buflen < 64) return UAPS_EINVAL;
    fwd_form_name(f, buf, buflen);
    return UAPS_OK;
}

namespace {
// the entry points below hand their arguments on as one FwdCall
int conv_fwd_any(const uaps_call_hints& h, const float* x, const float* wp, const float* bias, float* y, int B, int Cin, int Cout, int H, int W, int ks,
                 int cfg, hipStream_t s, float2* stats = nullptr, const float* x2 = nullptr, int Csplit = -1,
                 float* y2 = nullptr, int Osplit = -1, const void* xf = nullptr, float xf_slope = 0.f, int groups = 1) {
    const FwdCall c{x, wp, bias, y, B, Cin, Cout, H, W, ks, cfg, stats, x2, Csplit, y2, Osplit, xf, xf_slope, groups};
    return uaps::conv_fwd_run(h, c, s);
}
}  // namespace

static PackDesc make_pack_desc(const float* w, float* wf, float* wb, int Cout, int Cin, int ks) {
    PackDesc q{};
    q.w = w; q.wf = wf; q.wb = wb; q.Cout = Cout; q.Cin = Cin; q.taps = ks * ks;
    q.CinP = kdim_pad(Cin, ks); q.CoutP = ndim_pad(Cout); q.CoutPk = kdim_pad(Cout, ks); q.CinPn = ndim_pad(Cin);
    q.CGf = split_cgroups(Cin); q.CGb = split_cgroups(Cout);
    return q;
}

// Sizes (in floats) of the two packed buffers of a convolution: each holds the exact fp32 layout followed by the
// three-piece bf16 layout of conv_split.hpp (3 * taps * groups * channels * 16 bytes), a 16-byte header and the
// two-piece fp16 layout (2 * taps * groups * channels * 16 bytes).
extern "C" int uaps_conv_pack_floats(int Cout, int Cin, int ks, size_t* fwd_floats, size_t* bwd_floats) {
    if (Cout <= 0 || Cin <= 0 || (ks != 1 && ks != 3)) return UAPS_EINVAL;
    const size_t taps = (size_t)ks * ks;
    const PackDesc q = make_pack_desc(nullptr, nullptr, nullptr, Cout, Cin, ks);
    (void)taps;
    if (fwd_floats) *fwd_floats = (size_t)pack_fwd_floats(q);
    if (bwd_floats) *bwd_floats = (size_t)pack_bwd_floats(q);
    return UAPS_OK;
}

extern "C" int uaps_conv_pack_weights(const float* w, int Cout, int Cin, int ks, float* wf, float* wb, uaps_stream_t stream) {
    if (!w || Cout <= 0 || Cin <= 0 || (ks != 1 && ks != 3) || (!wf && !wb)) return UAPS_EINVAL;
    if (((uintptr_t)wf | (uintptr_t)wb) % 16) return UAPS_EINVAL;
    const PackDesc q = make_pack_desc(w, wf, wb, Cout, Cin, ks);
    const long n = conv_pack_elems(q);
    uaps::account_bytes(4.0 * ((double)Cout * Cin * ks * ks + (double)n));      // the weight once, every packed layout once
    const int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(conv_weight_scale_kernel, dim3(kH16Parts), dim3(256), 0, (hipStream_t)stream, q);
    hipLaunchKernelGGL(conv_pack_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, q);
    return (int)hipGetLastError();
}

// The same for n convolutions at once (host arrays of n entries each); any wf[i] / wb[i] may be null.
extern "C" int uaps_conv_pack_weights_batch(const float* const* w, float* const* wf, float* const* wb, const int* Cout,
                                            const int* Cin, const int* ks, int n, uaps_stream_t stream) {
    if (!w || !wf || !wb || !Cout || !Cin || !ks || n <= 0) return UAPS_EINVAL;
    for (int base = 0; base < n; base += kPackBatch) {
        const int m = n - base < kPackBatch ? n - base : kPackBatch;
        PackBatch pb{};
        long most = 0;
        for (int i = 0; i < m; ++i) {
            const int k = base + i;
            if (!w[k] || Cout[k] <= 0 || Cin[k] <= 0 || (ks[k] != 1 && ks[k] != 3)) return UAPS_EINVAL;
            if (((uintptr_t)wf[k] | (uintptr_t)wb[k]) % 16) return UAPS_EINVAL;
            pb.d[i] = make_pack_desc(w[k], wf[k], wb[k], Cout[k], Cin[k], ks[k]);
            const long e = conv_pack_elems(pb.d[i]);
            uaps::account_bytes(4.0 * ((double)Cout[k] * Cin[k] * ks[k] * ks[k] + (double)e));
            if (e > most) most = e;
        }
        const int bx = (int)((most + 255) / 256 < 256 ? (most + 255) / 256 : 256);
        hipLaunchKernelGGL(conv_weight_scale_batch_kernel, dim3(kH16Parts, m), dim3(256), 0, (hipStream_t)stream, pb);
        hipLaunchKernelGGL(conv_pack_weights_batch_kernel, dim3(bx, m), dim3(256), 0, (hipStream_t)stream, pb);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return UAPS_OK;
}

#ifdef UAPS_STAMPS
// diagnostic build only (stamps.hpp; not part of include/uaps_hip.h): where the stamped kernels of this file write, nwaves * 20 words
extern "C" int uaps_debug_set_stamp_buffer(unsigned long long* buf, unsigned long long nwaves) {
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(uaps::g_stamp_buf), &buf, sizeof buf);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(uaps::g_stamp_waves), &nwaves, sizeof nwaves);
    return (int)e;
}
#endif

// Every entry point below exists twice: `uaps_X(args)` takes its optional operands (bounds, statistics shift, ...) from the calling
// thread's pending uaps_next_call_hints record (the legacy form), `uaps_X_h(hints, args)` takes them as its first argument (NULL =
// none) and reads nothing thread-local (round 6: the form the Python package calls).
extern "C" int uaps_conv_fwd_h(const uaps_call_hints* hints, const float* x, const float* wf, const float* bias, float* y, int B, int Cin, int Cout,
                               int H, int W, int ks, int cfg, uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    return conv_fwd_any(h, x, wf, bias, y, B, Cin, Cout, H, W, ks, cfg, (hipStream_t)stream);
}
extern "C" int uaps_conv_fwd(const float* x, const float* wf, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                             int ks, int cfg, uaps_stream_t stream) {
    return conv_fwd_any(take_hints(), x, wf, bias, y, B, Cin, Cout, H, W, ks, cfg, (hipStream_t)stream);
}

// Forward convolution that also writes, per output channel, image and pixel tile, the (sum, sum of squares) of
// its output: the first pass of the train-mode BatchNorm that follows every 3x3 conv of a ConvBlock
// (UAPS_unet.py:37-38, 41-42), for uaps_bn_act_fwd_train_partials.  stats: float2 [Cout][B][parts_per_image].
extern "C" int uaps_conv_fwd_stats_h(const uaps_call_hints* hints, const float* x, const float* wf, const float* bias, float* y, void* stats,
                                     int B, int Cin, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    if (!stats) return UAPS_EINVAL;
    return conv_fwd_any(h, x, wf, bias, y, B, Cin, Cout, H, W, ks, cfg, (hipStream_t)stream, (float2*)stats);
}
extern "C" int uaps_conv_fwd_stats(const float* x, const float* wf, const float* bias, float* y, void* stats, int B, int Cin,
                                   int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream) {
    const uaps_call_hints h = take_hints();
    if (!stats) return UAPS_EINVAL;
    return conv_fwd_any(h, x, wf, bias, y, B, Cin, Cout, H, W, ks, cfg, (hipStream_t)stream, (float2*)stats);
}

// y = conv(leaky_relu(batch_norm_train(x_raw))) where x_raw is a previous conv's raw output and the normalisation
// coefficients xf [groups][Cin] float2 (scale, shift) come from uaps_bn_finalize_train: the activated
// tensor between the two convs of a ConvBlock (UAPS_unet.py:38-41) is never written.  stats may be NULL.
extern "C" int uaps_conv_fwd_bn_h(const uaps_call_hints* hints, const float* x_raw, const void* xf, float slope, int groups, const float* wf,
                                  const float* bias, float* y, void* stats, int B, int Cin, int Cout, int H, int W, int ks, int cfg,
                                  uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    if (!xf) return UAPS_EINVAL;
    return conv_fwd_any(h, x_raw, wf, bias, y, B, Cin, Cout, H, W, ks, cfg, (hipStream_t)stream, (float2*)stats, nullptr, -1, nullptr, -1,
                        xf, slope, groups);
}
extern "C" int uaps_conv_fwd_bn(const float* x_raw, const void* xf, float slope, int groups, const float* wf, const float* bias,
                                float* y, void* stats, int B, int Cin, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream) {
    const uaps_call_hints h = take_hints();
    if (!xf) return UAPS_EINVAL;
    return conv_fwd_any(h, x_raw, wf, bias, y, B, Cin, Cout, H, W, ks, cfg, (hipStream_t)stream, (float2*)stats, nullptr, -1, nullptr, -1,
                        xf, slope, groups);
}

extern "C" int uaps_conv_fwd_stats_parts(int B, int Cin, int Cout, int H, int W, int ks, int cfg, int* parts_per_image) {
    int parts = 0;
    const int rc = stats_parts(B, Cin, Cout, H, W, ks, cfg, &parts);
    if (rc) return rc;
    if (!parts_per_image) return UAPS_EINVAL;
    *parts_per_image = parts;
    return UAPS_OK;
}

// Convolution of the never-materialised concatenation torch.cat([x1, x2], dim=1) (UpBlock, UAPS_unet.py:84-85):
// x1 [B,C1,H,W], x2 [B,C2,H,W], weights packed for Cin = C1 + C2; C1 % 8 == 0.  stats may be NULL.
extern "C" int uaps_conv_fwd_cat_h(const uaps_call_hints* hints, const float* x1, int C1, const float* x2, int C2, const float* wf,
                                   const float* bias, float* y, void* stats, int B, int Cout, int H, int W, int ks, int cfg,
                                   uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    if (!x2 || C1 <= 0 || C2 <= 0) return UAPS_EINVAL;
    return conv_fwd_any(h, x1, wf, bias, y, B, C1 + C2, Cout, H, W, ks, cfg, (hipStream_t)stream, (float2*)stats, x2, C1);
}
extern "C" int uaps_conv_fwd_cat(const float* x1, int C1, const float* x2, int C2, const float* wf, const float* bias, float* y,
                                 void* stats, int B, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream) {
    const uaps_call_hints h = take_hints();
    if (!x2 || C1 <= 0 || C2 <= 0) return UAPS_EINVAL;
    return conv_fwd_any(h, x1, wf, bias, y, B, C1 + C2, Cout, H, W, ks, cfg, (hipStream_t)stream, (float2*)stats, x2, C1);
}

// Input gradient of that convolution, written as two tensors: dx1 [B,C1,H,W] and dx2 [B,C2,H,W].
extern "C" int uaps_conv_bwd_data_cat_h(const uaps_call_hints* hints, const float* dy, const float* wb, float* dx1, int C1, float* dx2, int C2,
                                        int B, int Cout, int H, int W, int ks, int cfg, uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    if (!dx2 || C1 <= 0 || C2 <= 0) return UAPS_EINVAL;
    return conv_fwd_any(h, dy, wb, nullptr, dx1, B, Cout, C1 + C2, H, W, ks, cfg, (hipStream_t)stream, nullptr, nullptr, -1, dx2, C1);
}
extern "C" int uaps_conv_bwd_data_cat(const float* dy, const float* wb, float* dx1, int C1, float* dx2, int C2, int B, int Cout,
                                      int H, int W, int ks, int cfg, uaps_stream_t stream) {
    const uaps_call_hints h = take_hints();
    if (!dx2 || C1 <= 0 || C2 <= 0) return UAPS_EINVAL;
    return conv_fwd_any(h, dy, wb, nullptr, dx1, B, Cout, C1 + C2, H, W, ks, cfg, (hipStream_t)stream, nullptr, nullptr, -1, dx2, C1);
}

// dx = conv(dy, W^T flipped): the same kernel with the roles of the channel counts exchanged
extern "C" int uaps_conv_bwd_data_h(const uaps_call_hints* hints, const float* dy, const float* wb, float* dx, int B, int Cin, int Cout, int H,
                                    int W, int ks, int cfg, uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    return conv_fwd_any(h, dy, wb, nullptr, dx, B, Cout, Cin, H, W, ks, cfg, (hipStream_t)stream);
}
extern "C" int uaps_conv_bwd_data(const float* dy, const float* wb, float* dx, int B, int Cin, int Cout, int H, int W, int ks,
                                  int cfg, uaps_stream_t stream) {
    return conv_fwd_any(take_hints(), dy, wb, nullptr, dx, B, Cout, Cin, H, W, ks, cfg, (hipStream_t)stream);
}

// Name of the kernel instantiation uaps_conv_fwd / uaps_conv_bwd_data launch for these dimensions (aligned tensors, no hints), as
// rocprofv3 prints it.  For bwd_data pass (Cout, Cin) swapped.  uaps_conv_ex_variant names the kernel of a whole call.
extern "C" int uaps_conv_fwd_variant(int B, int Cin, int Cout, int H, int W, int ks, int cfg, char* buf, size_t buflen) {
    const uaps_call_hints none{};
    const FwdCall c{nullptr, nullptr, nullptr, nullptr, B, Cin, Cout, H, W, ks, cfg};
    return conv_fwd_name(none, c, buf, buflen);
}
