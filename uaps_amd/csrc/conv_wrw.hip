// extern "C" entry points of the weight-gradient convolution (include/uaps_hip.h, "Convolutions").
#include "../../include/uaps_hip.h"
#include <stdio.h>
#include "conv_kernels.hpp"
#include "conv_split_wrw.hpp"
#include "conv_split_wrw_row.hpp"
#include "conv_small.hpp"
#include "conv_gemm1x1.hpp"
#include "hints.hpp"
#include "conv_call.hpp"
using namespace uaps;

extern "C" int uaps_conv_get_mode(void);
extern "C" unsigned uaps_conv_get_tuning(void);

namespace {

// wave arrangement: (WCO, WCI) 16-channel blocks per workgroup, the remaining factor of 4 splits the tile rows
// split: the bf16-split kernels of conv_split_wrw.hpp (3x3, no dilation, 16-byte rows, >= 16 input channels)
// g1: the GEMM-tiled 1x1 kernel of conv_gemm1x1.hpp (128 x 128 channel blocks, 32-pixel chunks)
struct WrwPlan { int TH, TW, wco, wci, ncob, ncib, nsplit, CoutS, CinS, dil; long tiles; bool split, small, g1; };

WrwPlan plan_wrw(int B, int Cin, int Cout, int H, int W, int cfg, int ks = 3) {
    WrwPlan p{};
    p.dil = ((cfg >> 24) & 0xf) ? ((cfg >> 24) & 0xf) : 1;       // bits 24-27: dilation; bit 28: exact kernels; bit 29: split kernels; low bits: pixel splits override
    const bool force_exact = (cfg >> 28) & 1, force_split = (cfg >> 29) & 1;
    cfg &= 0xffffff;
    p.split = ks == 3 && p.dil == 1 && W % 4 == 0 && !force_exact && (force_split || (uaps_conv_get_mode() >= 1 && Cin >= 16 && W >= 16));      // 32-pixel row tiles: half empty on 16-wide maps, still 1.2x the fp32 kernel there (256 -> 256 @16^2, B = 32: 97 -> 79 us)
    if (uaps_conv_get_tuning() & UAPS_TUNE_NO_SPLIT_WRW) p.split = false;
    // <= 4 output channels x 16 input channels on a wide map: the exact-N VALU kernel (conv_small.hpp), slabs [tap][4][16]
    p.small = ks == 3 && p.dil == 1 && W % 4 == 0 && W >= 64 && Cout <= 4 && Cin == 16 && !force_exact && !force_split;
    // wide 1x1 projections (ResNet bottlenecks): the same rule as plan_fwd's big_1x1
    p.g1 = ks == 1 && uaps_conv_get_mode() >= 1 && !force_exact && !(uaps_conv_get_tuning() & UAPS_TUNE_NO_SPLIT_WRW) && cfg == 0 &&
           Cin >= 64 && (long)Cin * Cout >= 16384 && (long)H * W >= 1024 && ((long)H * W) % 32 == 0 && W % 4 == 0;
    if (p.g1) {
        p.split = p.small = false;
        p.wco = p.wci = 8; p.TH = 1; p.TW = 32;
        p.ncob = (Cout + 127) / 128; p.ncib = (Cin + 127) / 128;
        p.CoutS = p.ncob * 128; p.CinS = p.ncib * 128;
        p.tiles = (long)B * (((long)H * W) / 32);
        const long blocks = (long)p.ncob * p.ncib;
        long want = blocks >= 1024 ? 1 : (1024 + blocks - 1) / blocks;      // ~4 workgroups per CU in all
        if (want > p.tiles) want = p.tiles;
        p.nsplit = (int)(want < 1 ? 1 : want);
        return p;
    }
    if (p.small) {
        p.split = false;
        p.wco = p.wci = 1; p.TH = 8; p.TW = 64; p.ncob = p.ncib = 1; p.CoutS = 4; p.CinS = 16;
        p.tiles = (long)B * ((H + p.TH - 1) / p.TH) * ((W + p.TW - 1) / p.TW);
        long want = cfg > 0 ? cfg : 512;
        if (want > p.tiles) want = p.tiles;
        p.nsplit = (int)(want < 1 ? 1 : want);
        return p;
    }
    if (p.split) {
        p.wco = Cout > 16 ? 2 : 1; p.wci = Cin > 16 ? 2 : 1;
        p.TH = 4; p.TW = 32;
        p.ncob = (Cout + 16 * p.wco - 1) / (16 * p.wco);
        p.ncib = (Cin + 16 * p.wci - 1) / (16 * p.wci);
        p.CoutS = p.ncob * 16 * p.wco; p.CinS = p.ncib * 16 * p.wci;
        p.tiles = (long)B * ((H + p.TH - 1) / p.TH) * ((W + p.TW - 1) / p.TW);
        const long blocks = (long)p.ncob * p.ncib;
        long want = blocks >= 512 ? 1 : 512 / blocks;
        if (cfg > 0) want = cfg;
        if (want > p.tiles) want = p.tiles;
        if (want < 1) want = 1;
        p.nsplit = (int)want;
        return p;
    }
    p.wco = Cout > 16 ? 2 : 1;
    p.wci = Cin > 16 ? 2 : 1;
    if (p.dil > 1) p.wco = p.wci = 2;                             // dilated variants exist for 32 x 32 channel blocks only
    const bool wide = W >= 32 || p.dil > 1, big = p.wco * p.wci == 4;     // 32x32 channel blocks stage half-height tiles (LDS)
    p.TW = wide ? 32 : 16;
    p.TH = wide ? (big ? 4 : 8) : (big ? 8 : 16);
    p.ncob = (Cout + 16 * p.wco - 1) / (16 * p.wco);
    p.ncib = (Cin + 16 * p.wci - 1) / (16 * p.wci);
    p.CoutS = p.ncob * 16 * p.wco; p.CinS = p.ncib * 16 * p.wci;
    p.tiles = (long)B * ((H + p.TH - 1) / p.TH) * ((W + p.TW - 1) / p.TW);
    // pixel splits: the kernels run two workgroups per CU (register-limited), so aim at exactly one round of
    // 512 equally loaded workgroups; more, smaller ones leave a half-empty second round and grow the slabs
    const long blocks = (long)p.ncob * p.ncib;
    long want = blocks >= 512 ? 1 : 512 / blocks;
    if (cfg > 0) want = cfg;
    if (want > p.tiles) want = p.tiles;
    if (want < 1) want = 1;
    p.nsplit = (int)want;
    return p;
}


size_t wrw_ws_floats(const WrwPlan& p, int taps) { return (size_t)p.nsplit * ((size_t)taps * p.CoutS * p.CinS + p.CoutS); }

// The kernel forms of the weight gradient; every one writes the slabs of the call's WrwPlan (workspace and reduction follow the plan)
enum class WrwKind {
    None,      // no form for the call's requests (dyt_*, UAPS_CONV_X2_UP2): check_wrw turns it into UAPS_ENOFORM
    Tile,      // conv_wrw_kernel<ks, th, tw, wco, wci, vec, dil>: the fp32 matrix instruction
    Small,     // conv_small_wrw_kernel: <= 4 output x 16 input channels (conv_small.hpp)
    G1,        // conv_gw1s / conv_gw1h_kernel: GEMM-tiled 1x1 (conv_gemm1x1.hpp)
    Split,     // conv_swrw / conv_hwrw_kernel<th, wco, wci> (conv_split_wrw.hpp)
    HwrwD,     // conv_hwrw_d_kernel<4, 2, 2, dil>: dilated, fp16 pieces
    Row,       // conv_hrwrw{,w,2,_up}_kernel<n>: full-width rows (conv_split_wrw_row.hpp), `_dt` with the dyt_* transform
};

struct WrwForm {
    WrwPlan plan;                       // the slab layout
    WrwKind kind;
    int ks, th, tw, wco, wci, dil, n;   // template parameters (Row: n = 1 / 2 for 16 / 32 input channels)
    bool vec, h16, bn, dt;              // 16-byte rows; fp16 pieces; staging-time BatchNorm; dy formed from dyt_*
    bool strips, deep, up;              // Row: 256-wide column strips, two row sets in flight, x2 up-sampled while staged
    bool up2;
    int Csplit;
    unsigned grid, block;
    int tiles_x, tiles_y;
};

// Which kernel the call runs: every condition of the choice, host code only (no HIP call)
int resolve_wrw(const uaps_call_hints& h, const WrwCall& c, WrwForm* out) {
    const int B = c.B, Cin = c.Cin, Cout = c.Cout, H = c.H, W = c.W, ks = c.ks;
    const void* xf = c.xf;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return UAPS_EINVAL;
    // UAPS_CONV_X2_UP2 (include/uaps_hip.h): x2 is [B, Cin - Csplit, H / 2, W / 2], up-sampled x2 while staged
    const bool up2 = (c.cfg & UAPS_CONV_X2_UP2) != 0;
    const int cfg = c.cfg & ~UAPS_CONV_X2_UP2;
    if (up2 && (!c.x2 || xf || H % 2 || W % 2)) return UAPS_EINVAL;
    if (xf && (c.x2 || c.groups < 1 || c.groups > kWrwMaxGroups || B % c.groups || (uintptr_t)xf % 8)) return UAPS_EINVAL;
    if (xf && !(c.xf_slope >= 0.f && c.xf_slope <= 1.f)) return UAPS_ERANGE;      // leaky_relu is evaluated as max(z, slope * z)
    const int Csplit = c.x2 ? c.Csplit : Cin;
    if (Csplit > Cin || (Csplit < Cin && (Csplit % 16 || Csplit == 0))) return UAPS_EINVAL;
    if (ks != 1 && ks != 3) return UAPS_ERANGE;
    if ((double)Cin * H * W * 4.0 >= 2147483648.0 || (double)Cout * H * W * 4.0 >= 2147483648.0) return UAPS_ERANGE;
    WrwForm f{};
    const WrwPlan& p = f.plan = plan_wrw(B, Cin, Cout, H, W, cfg, ks);
    const bool vec16 = (W % 4 == 0) && ((uintptr_t)c.x % 16 == 0) && ((uintptr_t)c.dy % 16 == 0) && (!c.x2 || (uintptr_t)c.x2 % 16 == 0);
    if ((p.split || p.small) && !vec16) return UAPS_ERANGE;      // the split kernels stream 16-byte pieces (W % 4 == 0 is part of the plan; pass cfg bit 28 for odd pointers)
    if (p.dil != 1 && (ks != 3 || (p.dil != 2 && p.dil != 4))) return UAPS_ERANGE;
    f.ks = ks; f.th = p.TH; f.tw = p.TW; f.wco = p.wco; f.wci = p.wci; f.dil = p.dil; f.vec = vec16; f.bn = xf != nullptr;
    f.up2 = up2; f.Csplit = Csplit;
    f.tiles_x = (W + p.TW - 1) / p.TW; f.tiles_y = (H + p.TH - 1) / p.TH;
    f.block = kConvThreads;
    const int mode = uaps_conv_get_mode();
    const unsigned tune = uaps_conv_get_tuning();
    const bool force_exact = (cfg >> 28) & 1;
    const bool dyt = h.dyt_y != nullptr;
    // full-width-row kernels (conv_split_wrw_row.hpp): maps of 256 pixels width or a multiple (256-wide column strips), <= 16 output and 16 / 32 input channels, every operand bounded;
    // they write the slabs of the plan above (split or exact-N), so workspace and reduction do not change
    // (fewer than 16 input channels -- the first layer's 3 -- ride in the 16-channel form: the absent channels are never fetched)
    if (ks == 3 && p.dil == 1 && !force_exact && vec16 && W % 256 == 0 && H % 16 == 0 && Cout <= 16 && Cin <= 32 &&
        p.CoutS <= 16 && p.CinS == (Cin > 16 ? 32 : 16) && p.ncob == 1 && p.ncib == 1 && mode == 2 && h.bound[0] && h.bound[1] &&
        (!c.x2 || Csplit >= Cin || (h.bound[2] && Csplit % 4 == 0)) && !(tune & (UAPS_TUNE_NO_ROW_WRW | UAPS_TUNE_NO_SPLIT_WRW))) {
        f.kind = WrwKind::Row; f.h16 = true; f.dt = dyt;
        f.n = Cin <= 16 ? 1 : 2;
        f.block = Cin <= 16 ? 256 : 512;
        if (up2) {                                     // up4's first convolution: 16 + 16 input channels, the second 16 from the low-resolution tensor
            f.up = true; f.block = 512;
            if (!(Cin == 32 && Csplit == 16 && W == 256 && uaps::up2_pattern_ok(W / 2))) f.kind = WrwKind::None;
        } else if (!dyt && (tune & UAPS_TUNE_DEEP_ROWS) && W == 256) {
            f.deep = true;                             // diagnostic: two rows in flight ahead of the contraction (measured slower)
        } else {
            f.strips = W > 256;
        }
    } else if (dyt || up2) {
        // (the tile kernels have no DT form: built and measured late in round 4 -- 32 x 32 channel blocks, bit-identical dy -- the extra
        // staging work cost them more than the stand-alone pass it replaced: 12 launches +314 us against 224 us saved)
        f.kind = WrwKind::None;
    } else if (p.g1) {
        // single-tensor, 16-byte-aligned form only; workspace and reduce follow the same plan, so the caller chooses: cfg bit 28
        // (exact kernels) for a two-tensor / BatchNorm-in-staging / odd-pointer call of such a layer -- uaps_amd.conv.plan_cfg does
        if (c.x2 || xf || !vec16) return UAPS_ERANGE;
        f.kind = WrwKind::G1;
        f.h16 = mode == 2 && h.bound[0] && h.bound[1];
        f.tiles_x = (H * W) / 32; f.tiles_y = 1;
    } else if (p.small) {
        if (c.x2) return UAPS_EINVAL;
        f.kind = WrwKind::Small;
    } else if (p.dil > 1 && ks == 3 && !xf && !c.x2 && vec16 && W >= 32 && Cin >= 16 && !force_exact && mode == 2 &&
               !(tune & UAPS_TUNE_NO_SPLIT_WRW) && h.bound[0] && h.bound[1] && p.wco == 2 && p.wci == 2 && p.TH == 4) {
        // dilated 3x3 with both operands bounded: the dilated fp16 form; same 32 x 32 channel blocks, 4-row tiles and slabs as the
        // fp32 kernel the plan describes, so workspace size and reduction are unchanged
        f.kind = WrwKind::HwrwD; f.h16 = true;
        f.tiles_y = p.dil * (((H + p.dil - 1) / p.dil + 3) / 4);      // per row phase: ceil(ceil(H / dil) / 4) tiles
        if ((long)B * f.tiles_x * f.tiles_y > 0x7fffffffL) return UAPS_EINVAL;
    } else if (p.split) {
        // mode 2 and every tensor operand bounded (0 = dy, 1 = x, 2 = x2): the two-piece fp16 form
        f.kind = WrwKind::Split;
        f.h16 = mode == 2 && h.bound[0] && h.bound[1] && (!c.x2 || Csplit >= Cin || h.bound[2]);
        // 16 output channels (the 256 x 256 level): 8-row tiles, halo rows 10/8 instead of 6/4 and half the barriers -- measured
        // 161 -> 150 us (32 -> 16 channels) and 103 -> 90 us (16 -> 16 with the staging-time BatchNorm) at B = 32; the 32 x 16 channel
        // block of the 128 x 128 level loses 10 % and keeps 4 rows
        if (f.h16 && p.wco == 1 && !(tune & UAPS_TUNE_WRW_SHORT_TILES) && H >= 8) {
            f.th = 8;
            f.tiles_y = (H + 7) / 8;
        }
    } else {
        f.kind = WrwKind::Tile;
        // the staging-time BatchNorm: 16-byte form, no dilation
        if (xf && (!vec16 || p.dil != 1)) return UAPS_ERANGE;
    }
    // the row and exact-N kernels take one workgroup per pixel split, the others one per split and channel block (a multiple of 8 for
    // the XCD swizzle)
    const long grid = ((long)p.nsplit * (f.kind == WrwKind::Row || f.kind == WrwKind::Small ? 1 : p.ncob * p.ncib) + 7) / 8 * 8;
    if (grid <= 0 || grid > 0x7fffffffL) return UAPS_EINVAL;
    f.grid = (unsigned)grid;
    *out = f;
    return UAPS_OK;
}

// The call's optional requests against its resolved form (nothing is launched when one fails)
int check_wrw(const uaps_call_hints& h, const WrwCall& c, const WrwForm& f) {
    // DT (uaps_call_hints::dyt_*): `dy` is d(activation) behind the BatchNorm that follows this convolution; only the row kernels
    // turn it into dy while staging
    if (h.dyt_y) {
        if (!h.dyt_coef || !h.dyt_out || h.dyt_groups < 1 || h.dyt_groups > kWrwMaxGroups || c.B % h.dyt_groups) return UAPS_EINVAL;
        if (!(h.dyt_slope >= 0.f && h.dyt_slope <= 1.f)) return UAPS_ERANGE;
        if (((uintptr_t)h.dyt_y | (uintptr_t)h.dyt_out) % 16) return UAPS_ENOFORM;      // the in-staging form streams 16-byte pieces
        if (f.kind != WrwKind::Row) return UAPS_ENOFORM;
    }
    if (f.up2 && !(f.kind == WrwKind::Row && f.up)) return UAPS_ENOFORM;
    return UAPS_OK;
}

// ---- the launch: a switch on the form (no choice is made below; the form names one instantiation) ----
using WrwKernel = void (*)(ConvWrwArgs);

template <int TH, int WCO, int WCI>
WrwKernel split_kernel(const WrwForm& f) {
    if constexpr (TH == 8) {
        return f.bn ? conv_hwrw_bn_kernel<8, WCO, WCI> : conv_hwrw_kernel<8, WCO, WCI>;
    } else {
        if (f.h16) return f.bn ? conv_hwrw_bn_kernel<4, WCO, WCI> : conv_hwrw_kernel<4, WCO, WCI>;
        return f.bn ? conv_swrw_bn_kernel<4, WCO, WCI> : conv_swrw_kernel<4, WCO, WCI>;
    }
}
template <int WCO, int WCI>
WrwKernel split_kernel_th(const WrwForm& f) {
    if constexpr (WCO == 1) {
        if (f.th == 8) return split_kernel<8, 1, WCI>(f);
    }
    return split_kernel<4, WCO, WCI>(f);
}

template <int KS, int TH, int TW, int WCO, int WCI, int DIL = 1>
WrwKernel tile_kernel(const WrwForm& f) {
    if constexpr (DIL == 1) {
        if (f.bn) return conv_wrw_bn_kernel<KS, TH, TW, WCO, WCI, 4, 1>;
    }
    return f.vec ? conv_wrw_kernel<KS, TH, TW, WCO, WCI, 4, DIL> : conv_wrw_kernel<KS, TH, TW, WCO, WCI, 1, DIL>;
}
template <int KS>
WrwKernel tile_kernel_ks(const WrwForm& f) {
    const bool wide = f.tw == 32;
    if constexpr (KS == 3) {
        if (f.dil == 2) return tile_kernel<3, 4, 32, 2, 2, 2>(f);
        if (f.dil == 4) return tile_kernel<3, 4, 32, 2, 2, 4>(f);
    }
    if (f.wco == 2 && f.wci == 2) return wide ? tile_kernel<KS, 4, 32, 2, 2>(f) : tile_kernel<KS, 8, 16, 2, 2>(f);
    if (f.wco == 2) return wide ? tile_kernel<KS, 8, 32, 2, 1>(f) : tile_kernel<KS, 16, 16, 2, 1>(f);
    if (f.wci == 2) return wide ? tile_kernel<KS, 8, 32, 1, 2>(f) : tile_kernel<KS, 16, 16, 1, 2>(f);
    return wide ? tile_kernel<KS, 8, 32, 1, 1>(f) : tile_kernel<KS, 16, 16, 1, 1>(f);
}

template <int N>
WrwKernel row_kernel(const WrwForm& f) {
    if (f.strips && f.dt) return f.bn ? conv_hrwrww_bn_dt_kernel<N> : conv_hrwrww_dt_kernel<N>;
    if (f.strips) return f.bn ? conv_hrwrww_bn_kernel<N> : conv_hrwrww_kernel<N>;
    if (f.deep) return f.bn ? conv_hrwrw2_bn_kernel<N> : conv_hrwrw2_kernel<N>;
    if (f.dt) return f.bn ? conv_hrwrw_bn_dt_kernel<N> : conv_hrwrw_dt_kernel<N>;
    return f.bn ? conv_hrwrw_bn_kernel<N> : conv_hrwrw_kernel<N>;
}

WrwKernel wrw_kernel(const WrwForm& f) {
    switch (f.kind) {
    case WrwKind::None: return nullptr;
    case WrwKind::Row:
        if (f.up) return f.dt ? conv_hrwrw_up_dt_kernel : conv_hrwrw_up_kernel;
        return f.n == 1 ? row_kernel<1>(f) : row_kernel<2>(f);
    case WrwKind::G1: return f.h16 ? conv_gw1h_kernel : conv_gw1s_kernel;
    case WrwKind::Small: return f.bn ? conv_small_wrw_bn_kernel : conv_small_wrw_kernel;
    case WrwKind::HwrwD: return f.dil == 2 ? conv_hwrw_d_kernel<4, 2, 2, 2> : conv_hwrw_d_kernel<4, 2, 2, 4>;
    case WrwKind::Split:
        if (f.wco == 2) return f.wci == 2 ? split_kernel_th<2, 2>(f) : split_kernel_th<2, 1>(f);
        return f.wci == 2 ? split_kernel_th<1, 2>(f) : split_kernel_th<1, 1>(f);
    case WrwKind::Tile: return f.ks == 3 ? tile_kernel_ks<3>(f) : tile_kernel_ks<1>(f);
    }
    return nullptr;
}

int launch_wrw(const uaps_call_hints& h, const WrwCall& c, const WrwForm& f, hipStream_t s) {
    const WrwPlan& p = f.plan;
    ConvWrwArgs a{};
    a.dout = c.dy; a.in = c.x; a.in2 = c.x2; a.Csplit = f.Csplit; a.slab = (float*)c.ws;
    a.B = c.B; a.Cin = c.Cin; a.Cout = c.Cout; a.H = c.H; a.W = c.W;
    a.CoutS = p.CoutS; a.CinS = p.CinS; a.tiles_x = f.tiles_x; a.tiles_y = f.tiles_y;
    a.col_major = (uaps_conv_get_tuning() & UAPS_TUNE_WRW_ROW_MAJOR) ? 0 : 1;      // column strips measured: 2.3x -> 1.07x of the algorithmic bytes at 32 -> 16 @ 256^2
    a.ncob = p.ncob; a.ncib = p.ncib; a.nsplit = p.nsplit;
    a.bslab = c.want_bias ? a.slab + (size_t)p.nsplit * c.ks * c.ks * p.CoutS * p.CinS : nullptr;
    a.xf = (const float2*)c.xf; a.xf_slope = c.xf_slope; a.xf_Bg = c.xf ? c.B / c.groups : c.B;
    if (h.dyt_y) { a.dt_y = h.dyt_y; a.dt_coef = h.dyt_coef; a.dt_out = h.dyt_out; a.dt_slope = h.dyt_slope; a.dt_Bg = c.B / h.dyt_groups; }
    if (f.h16) {
        a.dy_bound = h.bound[0]; a.dy_mul = h.mul[0];
        a.in_bound = h.bound[1]; a.in_mul = h.mul[1];
        if (c.x2 && f.Csplit < c.Cin) { a.in2_bound = h.bound[2]; a.in2_mul = h.mul[2]; }
        a.err = uaps::error_word();
    }
    if (f.up) { a.up_rh = (float)(c.H / 2 - 1) / (float)(c.H - 1); a.up_rw = (float)(c.W / 2 - 1) / (float)(c.W - 1); }      // as uaps_up_cat_fwd
    const WrwKernel k = wrw_kernel(f);
    if (!k) return UAPS_ENOFORM;
    UAPS_LAUNCH_MAIN(k, dim3(f.grid), dim3(f.block), 0, s, a);
    return (int)hipGetLastError();
}

// the rocprofv3 name of a form's kernel (without namespace)
void wrw_form_name(const WrwForm& f, char* buf, size_t len) {
    const char* bn = f.bn ? "_bn" : "";
    switch (f.kind) {
    case WrwKind::None: buf[0] = 0; break;
    case WrwKind::Tile: snprintf(buf, len, "conv_wrw%s_kernel<%d, %d, %d, %d, %d, %d, %d>", bn, f.ks, f.th, f.tw, f.wco, f.wci, f.vec ? 4 : 1, f.dil); break;
    case WrwKind::Small: snprintf(buf, len, "conv_small_wrw%s_kernel", bn); break;
    case WrwKind::G1: snprintf(buf, len, "conv_gw1%c_kernel", f.h16 ? 'h' : 's'); break;
    case WrwKind::Split: snprintf(buf, len, "conv_%cwrw%s_kernel<%d, %d, %d>", f.h16 ? 'h' : 's', bn, f.th, f.wco, f.wci); break;
    case WrwKind::HwrwD: snprintf(buf, len, "conv_hwrw_d_kernel<4, 2, 2, %d>", f.dil); break;
    case WrwKind::Row:
        if (f.up) snprintf(buf, len, "conv_hrwrw_up%s_kernel", f.dt ? "_dt" : "");
        else snprintf(buf, len, "conv_hrwrw%s%s%s_kernel<%d>", f.strips ? "w" : f.deep ? "2" : "", bn, f.dt ? "_dt" : "", f.n);
        break;
    }
}

}  // namespace

int uaps::conv_wrw_run(const uaps_call_hints& h, const WrwCall& c, uaps_stream_t stream) {
    if (!c.dy || !c.x || !c.ws) return UAPS_EINVAL;
    WrwForm f;
    int rc = resolve_wrw(h, c, &f);
    if (rc) return rc;
    if (c.ws_bytes < wrw_ws_floats(f.plan, c.ks * c.ks) * sizeof(float)) return UAPS_EWORKSPACE;
    // dy and x once each (+ the raw output read and the true dy written through when the call carries a pending BatchNorm transform)
    uaps::account_bytes(4.0 * c.B * c.H * c.W *
                        ((double)f.Csplit + (c.Cin - f.Csplit) * (f.up2 ? 0.25 : 1.0) + c.Cout + (h.dyt_y ? 2.0 * c.Cout : 0.0)));
    rc = check_wrw(h, c, f);
    if (rc) return rc;
    return launch_wrw(h, c, f, (hipStream_t)stream);
}

int uaps::conv_wrw_name(const uaps_call_hints& h, const WrwCall& c, char* buf, size_t buflen) {
    WrwForm f;
    int rc = resolve_wrw(h, c, &f);
    if (!rc) rc = check_wrw(h, c, f);
    if (rc) return rc;
    if (!buf || buflen < 64) return UAPS_EINVAL;
    wrw_form_name(f, buf, buflen);
    return UAPS_OK;
}

extern "C" int uaps_conv_wrw_workspace_bytes(int B, int Cin, int Cout, int H, int W, int ks, int cfg, size_t* out) {
    if (!out || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (ks != 1 && ks != 3)) return UAPS_EINVAL;
    *out = wrw_ws_floats(plan_wrw(B, Cin, Cout, H, W, cfg, ks), ks * ks) * sizeof(float);
    return UAPS_OK;
}

// the entry points below hand their arguments on as one WrwCall
static int wrw_partial_impl(const uaps_call_hints& hints, const float* dy, const float* x, const float* x2, int Csplit, int want_bias, int B, int Cin, int Cout,
                            int H, int W, int ks, int cfg, void* ws, size_t ws_bytes, uaps_stream_t stream,
                            const void* xf = nullptr, float xf_slope = 0.f, int groups = 1) {
    const WrwCall c{dy, x, x2, Csplit, want_bias, B, Cin, Cout, H, W, ks, cfg, ws, ws_bytes, xf, xf_slope, groups};
    return uaps::conv_wrw_run(hints, c, stream);
}


// (each entry point twice: the legacy form reads the thread's pending uaps_next_call_hints record, the *_h form takes the record as
// its first argument and reads nothing thread-local -- see conv_fwd.hip)
extern "C" int uaps_conv_bwd_weight_partial_h(const uaps_call_hints* hints, const float* dy, const float* x, int want_bias, int B, int Cin,
                                              int Cout, int H, int W, int ks, int cfg, void* ws, size_t ws_bytes, uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    return wrw_partial_impl(h, dy, x, nullptr, Cin, want_bias, B, Cin, Cout, H, W, ks, cfg, ws, ws_bytes, stream);
}
extern "C" int uaps_conv_bwd_weight_partial(const float* dy, const float* x, int want_bias, int B, int Cin, int Cout, int H, int W,
                                            int ks, int cfg, void* ws, size_t ws_bytes, uaps_stream_t stream) {
    return wrw_partial_impl(uaps::take_hints(), dy, x, nullptr, Cin, want_bias, B, Cin, Cout, H, W, ks, cfg, ws, ws_bytes, stream);
}

// Weight gradient of a convolution whose input is leaky_relu(batch_norm_train(y)) of a previous conv's raw output y
// (ConvBlock, UAPS_unet.py:38-41): the activation is recomputed while staging from xf [groups][Cin] float2
// (scale, shift) as uaps_bn_finalize_train wrote it.  W % 4 == 0, 16-byte aligned tensors.
extern "C" int uaps_conv_bwd_weight_partial_bn_h(const uaps_call_hints* hints, const float* dy, const float* y, const void* xf, float slope,
                                                 int groups, int want_bias, int B, int Cin, int Cout, int H, int W, int ks, int cfg,
                                                 void* ws, size_t ws_bytes, uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    if (!xf) return UAPS_EINVAL;
    return wrw_partial_impl(h, dy, y, nullptr, Cin, want_bias, B, Cin, Cout, H, W, ks, cfg, ws, ws_bytes, stream, xf, slope, groups);
}
extern "C" int uaps_conv_bwd_weight_partial_bn(const float* dy, const float* y, const void* xf, float slope, int groups,
                                               int want_bias, int B, int Cin, int Cout, int H, int W, int ks, int cfg, void* ws,
                                               size_t ws_bytes, uaps_stream_t stream) {
    const uaps_call_hints h = uaps::take_hints();
    if (!xf) return UAPS_EINVAL;
    return wrw_partial_impl(h, dy, y, nullptr, Cin, want_bias, B, Cin, Cout, H, W, ks, cfg, ws, ws_bytes, stream, xf, slope, groups);
}

// Weight gradient of a convolution whose input is the never-materialised concatenation of x1 [B,C1,H,W] and
// x2 [B,C2,H,W] (C1 % 16 == 0); follow with uaps_conv_bwd_weight_reduce(..., Cin = C1 + C2, ...).
extern "C" int uaps_conv_bwd_weight_partial_cat_h(const uaps_call_hints* hints, const float* dy, const float* x1, int C1, const float* x2, int C2,
                                                  int want_bias, int B, int Cout, int H, int W, int ks, int cfg, void* ws, size_t ws_bytes,
                                                  uaps_stream_t stream) {
    UAPS_READ_HINTS(hints, h);
    if (!x2 || C1 <= 0 || C2 <= 0) return UAPS_EINVAL;
    return wrw_partial_impl(h, dy, x1, x2, C1, want_bias, B, C1 + C2, Cout, H, W, ks, cfg, ws, ws_bytes, stream);
}
extern "C" int uaps_conv_bwd_weight_partial_cat(const float* dy, const float* x1, int C1, const float* x2, int C2, int want_bias,
                                                int B, int Cout, int H, int W, int ks, int cfg, void* ws, size_t ws_bytes,
                                                uaps_stream_t stream) {
    const uaps_call_hints h = uaps::take_hints();
    if (!x2 || C1 <= 0 || C2 <= 0) return UAPS_EINVAL;
    return wrw_partial_impl(h, dy, x1, x2, C1, want_bias, B, C1 + C2, Cout, H, W, ks, cfg, ws, ws_bytes, stream);
}

// Step 2: fixed-order sum of the partials into dw (and dbias).
extern "C" int uaps_conv_bwd_weight_reduce(const void* ws, float* dw, float* dbias, int B, int Cin, int Cout, int H, int W, int ks,
                                           int cfg, uaps_stream_t stream) {
    if (!ws || !dw || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (ks != 1 && ks != 3)) return UAPS_EINVAL;
    const int taps = ks * ks;
    const WrwPlan p = plan_wrw(B, Cin, Cout, H, W, cfg, ks);
    const float* slab = (const float*)ws;
    const float* bslab = dbias ? slab + (size_t)p.nsplit * taps * p.CoutS * p.CinS : nullptr;
    hipStream_t s = (hipStream_t)stream;
    const long n = (long)taps * p.CoutS * p.CinS + (dbias ? p.CoutS : 0);
    if (n < 32768)
        hipLaunchKernelGGL(conv_wrw_reduce_kernel<16>, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, slab, bslab, dw, dbias,
                           p.nsplit, taps, Cout, Cin, p.CoutS, p.CinS);
    else
        hipLaunchKernelGGL(conv_wrw_reduce_kernel<64>, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, slab, bslab, dw, dbias,
                           p.nsplit, taps, Cout, Cin, p.CoutS, p.CinS);
    return (int)hipGetLastError();
}

// Step 2 for several weight gradients at once: item i is reduced exactly as uaps_conv_bwd_weight_reduce(items[i]...) would
// (bit-identical), by one launch per kReduceBatch items.  The workspaces must be distinct and stay untouched until this call.
extern "C" int uaps_conv_bwd_weight_reduce_batch(const uaps_wrw_reduce_item* items, int n, uaps_stream_t stream) {
    if (n < 0 || (n > 0 && !items)) return UAPS_EINVAL;
    for (int i = 0; i < n; ++i) {
        const uaps_wrw_reduce_item& it = items[i];
        if (!it.workspace || !it.dw || it.B <= 0 || it.Cin <= 0 || it.Cout <= 0 || it.H <= 0 || it.W <= 0 || (it.ks != 1 && it.ks != 3)) return UAPS_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    for (int i0 = 0; i0 < n; i0 += kReduceBatch) {
        ReduceBatch rb{};
        unsigned blocks = 0;
        const int m = n - i0 < kReduceBatch ? n - i0 : kReduceBatch;
        for (int j = 0; j < m; ++j) {
            const uaps_wrw_reduce_item& it = items[i0 + j];
            const int taps = it.ks * it.ks;
            const WrwPlan p = plan_wrw(it.B, it.Cin, it.Cout, it.H, it.W, it.cfg, it.ks);
            ReduceDesc& q = rb.d[j];
            q.slab = (const float*)it.workspace;
            q.bslab = it.dbias ? q.slab + (size_t)p.nsplit * taps * p.CoutS * p.CinS : nullptr;
            q.dw = it.dw; q.db = it.dbias;
            q.nsplit = p.nsplit; q.taps = taps; q.Cout = it.Cout; q.Cin = it.Cin; q.CoutS = p.CoutS; q.CinS = p.CinS;
            const long ne = (long)taps * p.CoutS * p.CinS + (it.dbias ? p.CoutS : 0);
            q.el = ne < 32768 ? 16 : 64;
            q.first = blocks;
            long nb = (ne + q.el - 1) / q.el;
            const long nw = (long)taps * p.CoutS * p.CinS;
            if (q.el == 64 && nw % 4 == 0 && (reinterpret_cast<uintptr_t>(q.slab) & 15) == 0) {      // the 16-byte form of conv_wrw_reduce_batch_kernel
                q.el = 256;
                nb = (nw + 255) / 256 + (it.dbias ? (p.CoutS + 63) / 64 : 0);
            }
            if (nb + blocks > 0x7fffffffL) return UAPS_ERANGE;
            blocks += (unsigned)nb;
        }
        rb.n = m; rb.blocks = blocks;
        hipLaunchKernelGGL(conv_wrw_reduce_batch_kernel, dim3(blocks), dim3(256), 0, s, rb);
    }
    return (int)hipGetLastError();
}

extern "C" int uaps_conv_bwd_weight(const float* dy, const float* x, float* dw, float* dbias, int B, int Cin, int Cout, int H,
                                    int W, int ks, int cfg, void* ws, size_t ws_bytes, uaps_stream_t stream) {
    if (!dw) return UAPS_EINVAL;
    const int rc = uaps_conv_bwd_weight_partial(dy, x, dbias != nullptr, B, Cin, Cout, H, W, ks, cfg, ws, ws_bytes, stream);
    if (rc) return rc;
    return uaps_conv_bwd_weight_reduce(ws, dw, dbias, B, Cin, Cout, H, W, ks, cfg, stream);
}

// Name of the kernel instantiation uaps_conv_bwd_weight_partial launches for these dimensions (aligned tensors, no hints)
extern "C" int uaps_conv_wrw_variant(int B, int Cin, int Cout, int H, int W, int ks, int cfg, char* buf, size_t buflen) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (ks != 1 && ks != 3) || !buf || buflen < 64) return UAPS_EINVAL;
    const uaps_call_hints none{};
    const WrwCall c{nullptr, nullptr, nullptr, Cin, 0, B, Cin, Cout, H, W, ks, cfg};
    return conv_wrw_name(none, c, buf, buflen);
}
