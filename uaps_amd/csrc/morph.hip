// Mask clean-up morphology for gfx950 (include/uaps_hip.h, uaps_morphology): a chain of erode / dilate / open / close / boundary steps
// on an int64 label map [B,H,W] in ONE launch that reads the map once and writes it once.
//
// A workgroup owns a tile of `band` rows x `tw` 64-pixel words of one image and stages it with a halo of `reach` rows above and below
// and, where the image is wider than the tile, one word (64 >= reach pixels) left and right.  On wave64 a ballot of `mask == c` over 64
// consecutive pixels IS the bit word of class c, so staging turns the map into bit planes in LDS: one per selected class (P), one
// "occupied by a value that is neither selected nor the background" plane (O).  Every step then runs on those planes:
//   primitive   out[y] = AND / OR over dy of span(src[y + dy], w(|dy|)): the footprint is a union of centred row runs, w the table of
//               half-widths.  Rows +dy and -dy share a half-width and so do neighbouring |dy| of a square or a disk: their words are
//               combined FIRST (AND and the span commute), and one span is formed per distinct half-width.  A span of half-width w is
//               a run of 2w + 1 bits over the 128-bit window (previous, this, next word) shifted by w, built by doubling the run
//               length: at most five shift-and-combine stages for w <= 15.
//   neutral     rows and words outside the IMAGE and the tail bits of the last word read as the primitive's neutral element (1 for
//               erosion, 0 for dilation) at every read: stored planes keep their tail bits 0 and nothing stored outside the image is
//               ever used.  Rows and words outside the STAGED tile read as neutral too; what that spoils moves inwards by the radius
//               per primitive and `reach` is the sum of the radii, so it ends before the owned rows and words.
//   combine     erode / open / boundary shrink every plane inside itself and the planes are disjoint: P_c := R_c (boundary: P_c & ~R_c).
//               dilate / close only grow (both are extensive under the border rule): kept pixels are P_c itself, and the free pixels
//               F = ~O & ~(P_0 | ... ) go to the smallest class whose result covers them -- classes are visited in ascending order and
//               every visited result is struck from F.
// The A / T result planes exist for G classes at a time (G = all of them wherever that fits): n + 2 + 2G planes of R x sw words, at
// most 64 KiB.  No atomics, no scratch, integer work only; a pixel's result does not depend on the tiling.
#include "call_common.hpp"

namespace {
using uaps::kThreads; using uaps::kWaves; using uaps::kTooBig; using uaps::u64;

constexpr int kMaxSteps = 8, kMaxSel = 8, kMaxRadius = 15, kMaxReach = 64, kMaxExtent = 4096;
constexpr int kLdsWords = 64 * 1024 / 8;       // the plane budget of a workgroup, in 64-bit words
constexpr int kMaxTileWords = 8;                // a tile is at most 512 pixels wide
constexpr int kStage = 8;                       // words a wave stages per round

struct MorphArgs {
    int B, H, W, nw;            // nw: words of a row
    int n, G;                   // selected classes (ascending), classes per group of result planes
    int band, R, reach;         // owned rows, staged rows = band + 2 reach
    int tw, sw, hx, ntx, nby;   // owned words, staged words = tw + 2 hx, halo words per side (0 | 1), tiles per row, bands per image
    int n_steps;
    int op[kMaxSteps], radius[kMaxSteps];
    u64 hw[kMaxSteps];          // the footprint's half-width at |dy| = d in bits [4d, 4d + 4): a table that lives in two scalar registers
    long long cls[kMaxSel], bg;
    const long long* mask;
    long long* out;
};

struct Tile { int R, sw, H, nw, ry0, gj0; u64 tail; };   // ry0 / gj0: image row / word of the staged tile's first row / word

// bit x of the result: AND (E) or OR over the bits x - w .. x + w of the row whose words around this one are p, c, n
template <bool E>
__device__ __forceinline__ u64 span(u64 p, u64 c, u64 n, int w) {
    if (w == 0) return c;
    u64 lo = (p >> (64 - w)) | (c << w), hi = (c >> (64 - w)) | (n << w);   // the window from bit -w of this word on
    const int L = 2 * w + 1;
    int k = 1;                                  // (lo, hi) holds runs of length k; only bits below 64 + 2w of them are ever used
    for (; 2 * k <= L; k *= 2) {
        const u64 slo = (lo >> k) | (hi << (64 - k)), shi = hi >> k;
        lo = E ? lo & slo : lo | slo;
        hi = E ? hi & shi : hi | shi;
    }
    if (k < L) {
        const int s = L - k;
        const u64 slo = (lo >> s) | (hi << (64 - s));
        lo = E ? lo & slo : lo | slo;
    }
    return lo;
}

__device__ __forceinline__ int half_width(u64 hw, int d) { return (int)((hw >> (4 * d)) & 15); }

// dst[k] := src[k] eroded (E) or dilated by the footprint hw (half_width(hw, 0 .. r)), rows [lo, hi) of nk planes (plane stride ps on
// both sides)
template <bool E>
__device__ __forceinline__ void primitive(const u64* src, u64* dst, int nk, int ps, const Tile& t, int lo, int hi, int r,
                                          u64 hw) {
    const u64 neutral = E ? ~0ull : 0ull;
    const int per = (hi - lo) * t.sw, total = nk * per;
    for (int it = threadIdx.x; it < total; it += kThreads) {
        const int k = it / per, rem = it - k * per, lr = lo + rem / t.sw, lj = rem % t.sw;
        const u64* pl = src + k * ps;
        // the three words of a source row: which of them exist (staged and inside the image; the others read as neutral), and which
        // is the image's last word (its tail bits read as neutral too).  Loads are unconditional, from a clamped index.
        const int gj = t.gj0 + lj;
        const bool cL = lj > 0 && gj > 0 && gj <= t.nw, cM = gj >= 0 && gj < t.nw, cR = lj + 1 < t.sw && gj + 1 >= 0 && gj + 1 < t.nw;
        const int jL = cL ? lj - 1 : lj, jR = cR ? lj + 1 : lj;
        const u64 oL = (E && gj == t.nw) ? ~t.tail : 0ull, oM = (E && gj == t.nw - 1) ? ~t.tail : 0ull, oR = (E && gj == t.nw - 2) ? ~t.tail : 0ull;
        u64 res = neutral, a0 = neutral, a1 = neutral, a2 = neutral;
        for (int d = 0; d <= r; ++d) {
            for (int s = 0; s < (d ? 2 : 1); ++s) {
                const int y = s ? lr + d : lr - d, iy = t.ry0 + y;
                if (y < 0 || y >= t.R || iy < 0 || iy >= t.H) continue;       // a row that is not there: neutral
                const u64* row = pl + y * t.sw;
                const u64 r0 = row[jL], r1 = row[lj], r2 = row[jR];
                const u64 v0 = cL ? r0 | oL : neutral, v1 = cM ? r1 | oM : neutral, v2 = cR ? r2 | oR : neutral;
                a0 = E ? a0 & v0 : a0 | v0;
                a1 = E ? a1 & v1 : a1 | v1;
                a2 = E ? a2 & v2 : a2 | v2;
            }
            if (d == r || half_width(hw, d + 1) != half_width(hw, d)) {
                const u64 v = span<E>(a0, a1, a2, half_width(hw, d));
                res = E ? res & v : res | v;
                a0 = a1 = a2 = neutral;
            }
        }
        dst[k * ps + lr * t.sw + lj] = (gj == t.nw - 1) ? res & t.tail : res;
    }
}

__global__ __launch_bounds__(kThreads) void morph_chain_kernel(MorphArgs a) {
    extern __shared__ u64 lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long blk = blockIdx.x;
    const int tx = (int)(blk % a.ntx);
    const long rest = blk / a.ntx;
    const int by = (int)(rest % a.nby), b = (int)(rest / a.nby);
    Tile t;
    t.R = a.R; t.sw = a.sw; t.H = a.H; t.nw = a.nw;
    t.ry0 = by * a.band - a.reach;
    t.gj0 = tx * a.tw - a.hx;
    t.tail = (a.W & 63) ? (1ull << (a.W & 63)) - 1 : ~0ull;
    const int ps = a.R * a.sw, n = a.n;
    u64* P = lds;
    u64* O = P + n * ps;
    u64* F = O + ps;
    u64* A = F + ps;
    u64* T = A + a.G * ps;
    const long HW = (long)a.H * a.W;
    const long long* m = a.mask + (long)b * HW;

    long long cls[kMaxSel];                     // (static indices below: the classes stay in scalar registers)
#pragma unroll
    for (int k = 0; k < kMaxSel; ++k) cls[k] = a.cls[k];
    // the tile and its halo -> bit planes: one wave per word, one ballot per plane; kStage loads of a wave are in flight together
    for (int base = wave; base < ps; base += kWaves * kStage) {
        long long v[kStage];
        bool in[kStage];
#pragma unroll
        for (int q = 0; q < kStage; ++q) {
            const int it = base + q * kWaves, lr = it / a.sw, lj = it - lr * a.sw;
            const int iy = t.ry0 + lr, gj = t.gj0 + lj, x = gj * 64 + lane;
            in[q] = it < ps && iy >= 0 && iy < a.H && gj >= 0 && x < a.W;
            v[q] = a.bg;
            if (in[q]) v[q] = m[(long)iy * a.W + x];
        }
#pragma unroll
        for (int q = 0; q < kStage; ++q) {
            const int it = base + q * kWaves;
            if (it >= ps) break;                  // (wave-uniform)
            bool sel = false;
#pragma unroll
            for (int k = 0; k < kMaxSel; ++k) {
                if (k >= n) break;
                const bool e = in[q] && v[q] == cls[k];
                const u64 word = __ballot(e);
                if (lane == k) P[k * ps + it] = word;
                sel |= e;
            }
            const u64 word = __ballot(in[q] && !sel && v[q] != a.bg);
            if (lane == n) O[it] = word;
        }
    }
    __syncthreads();

    int u = 0;                                  // rows at either end of the staged tile that no longer hold the step's input
    for (int s = 0; s < a.n_steps; ++s) {
        const int op = a.op[s], r = a.radius[s];
        const u64 hw = a.hw[s];
        const bool two = op == UAPS_MORPH_OPEN || op == UAPS_MORPH_CLOSE;
        const bool grow = op == UAPS_MORPH_DILATE || op == UAPS_MORPH_CLOSE;
        const int u1 = u + r, u2 = two ? u1 + r : u1;
        const int w0 = u2 * a.sw, w1 = (a.R - u2) * a.sw;
        if (grow)
            for (int it = w0 + threadIdx.x; it < w1; it += kThreads) {
                u64 occ = O[it];
                for (int k = 0; k < n; ++k) occ |= P[k * ps + it];
                F[it] = ~occ;
            }
        for (int g0 = 0; g0 < n; g0 += a.G) {
            const int nk = n - g0 < a.G ? n - g0 : a.G;
            const u64* src = P + g0 * ps;
            if (two) {
                if (grow) primitive<false>(src, A, nk, ps, t, u1, a.R - u1, r, hw);
                else primitive<true>(src, A, nk, ps, t, u1, a.R - u1, r, hw);
                __syncthreads();
                if (grow) primitive<true>(A, T, nk, ps, t, u2, a.R - u2, r, hw);
                else primitive<false>(A, T, nk, ps, t, u2, a.R - u2, r, hw);
            } else {
                if (grow) primitive<false>(src, T, nk, ps, t, u1, a.R - u1, r, hw);
                else primitive<true>(src, T, nk, ps, t, u1, a.R - u1, r, hw);
            }
            __syncthreads();
            for (int it = w0 + threadIdx.x; it < w1; it += kThreads) {      // (the same lane owns word `it` of F in every pass)
                if (grow) {
                    u64 f = F[it];
                    for (int k = 0; k < nk; ++k) {
                        const u64 v = T[k * ps + it];
                        P[(g0 + k) * ps + it] |= v & f;
                        f &= ~v;
                    }
                    F[it] = f;
                } else {
                    for (int k = 0; k < nk; ++k) {
                        const u64 v = T[k * ps + it];
                        u64* p = P + (g0 + k) * ps + it;
                        *p = op == UAPS_MORPH_BOUNDARY ? *p & ~v : v;
                    }
                }
            }
            __syncthreads();
        }
        u = u2;
    }

    // the owned rows and words -> int64: one wave per word
    long long* out = a.out + (long)b * HW;
    for (int it = wave; it < a.band * a.tw; it += kWaves) {
        const int lr = a.reach + it / a.tw, lj = a.hx + it % a.tw;
        const int iy = t.ry0 + lr, gj = t.gj0 + lj, x = gj * 64 + lane;
        if (iy >= a.H || gj >= a.nw) continue;      // (wave-uniform; iy >= 0 and gj >= 0 for what a tile owns)
        if (x >= a.W) continue;
        const int idx = lr * a.sw + lj;
        long long v = a.bg;
        bool found = false;
#pragma unroll
        for (int k = 0; k < kMaxSel; ++k) {
            if (k >= n) break;
            if ((P[k * ps + idx] >> lane) & 1) { v = cls[k]; found = true; }
        }
        const long px = (long)iy * a.W + x;
        if (!found && ((O[idx] >> lane) & 1)) v = m[px];          // values the chain never touches pass through
        out[px] = v;
    }
}

struct Plan { int band, tw, hx, sw, ntx, G; };

// The tiling of an H x W image with n selected classes under a chain of the given reach; forced > 0: that band height.
//   tile width   the whole row up to kMaxTileWords words, halved until the planes fit
//   groups       all n result planes at once, halved until the planes fit (at a width, groups shrink before the width does)
//   band height  what fits in the budget, at most clamp(reach / 2, 8, 32) rows, evened out over the bands of the image.  Short bands
//                although the halo then is several times the band: a workgroup runs its phases one after the other with one wave per
//                SIMD, so the kernel is bound by how many workgroups the chip holds at once, not by the halo's extra words (measured
//                at 16 x 256 x 256 and 2 x 1024 x 1024, DESIGN.md section 3.24: 8 rows beat 16 and 32 for every chain timed).
//   A tiling is taken only where at least min(H, 8) rows fit; the narrowest one (one word, one class at a time, 12 planes of 3 words
//   a row) fits 99 rows at reach 64, so every chain the entry point admits has a tiling.
int make_plan(int H, int W, int n, int reach, int forced, Plan& p) {
    const int nw = (W + 63) / 64;
    const int need = forced > 0 ? forced : (H < 8 ? H : 8);
    for (int tw = nw < kMaxTileWords ? nw : kMaxTileWords; tw >= 1; tw /= 2) {
        const int hx = tw < nw ? 1 : 0, sw = tw + 2 * hx;
        for (int G = n; G >= 1; G /= 2) {
            const int fit = kLdsWords / ((n + 2 + 2 * G) * sw) - 2 * reach;
            if (fit < need) continue;
            int band = forced;
            if (forced <= 0) {
                const int cap = reach / 2 < 8 ? 8 : (reach / 2 > 32 ? 32 : reach / 2);
                band = fit < cap ? fit : cap;
                if (band > H) band = H;
                const int nb = (H + band - 1) / band;
                band = (H + nb - 1) / nb;
            }
            p.band = band; p.tw = tw; p.hx = hx; p.sw = sw; p.ntx = (nw + tw - 1) / tw; p.G = G;
            return UAPS_OK;
        }
    }
    return UAPS_ERANGE;
}
}  // namespace

extern "C" int uaps_morph_band_rows(int H, int W, int n_planes, int reach, int* rows) {
    if (!rows || H <= 0 || W <= 0 || n_planes < 2 || n_planes > kMaxSel + 1 || reach < 1) return UAPS_EINVAL;
    if (H > kMaxExtent || W > kMaxExtent || reach > kMaxReach) return UAPS_ERANGE;
    Plan p;
    const int rc = make_plan(H, W, n_planes - 1, reach, 0, p);
    if (rc) return rc;
    *rows = p.band;
    return UAPS_OK;
}

extern "C" int uaps_morphology(const uaps_morph_call* call) {
    uaps_morph_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.mask || !c.out || (const void*)c.out == (const void*)c.mask) return UAPS_EINVAL;
    if (c.B <= 0 || c.H <= 0 || c.W <= 0) return UAPS_EINVAL;
    if (c.n_steps < 1 || c.n_steps > kMaxSteps || c.n_classes < 1 || c.n_classes > kMaxSel || c.band_rows < 0) return UAPS_EINVAL;
    for (int s = 0; s < c.n_steps; ++s)
        if (c.op[s] < UAPS_MORPH_ERODE || c.op[s] > UAPS_MORPH_BOUNDARY || c.footprint[s] < UAPS_MORPH_SQUARE || c.footprint[s] > UAPS_MORPH_DISK)
            return UAPS_EINVAL;
    if (!uaps::distinct_classes(c.classes, c.n_classes, c.background)) return UAPS_EINVAL;
    int reach = 0;
    for (int s = 0; s < c.n_steps; ++s) {
        if (c.radius[s] < 1 || c.radius[s] > kMaxRadius) return UAPS_ERANGE;
        reach += (c.op[s] == UAPS_MORPH_OPEN || c.op[s] == UAPS_MORPH_CLOSE) ? 2 * c.radius[s] : c.radius[s];
    }
    if (reach > kMaxReach || c.H > kMaxExtent || c.W > kMaxExtent) return UAPS_ERANGE;
    if ((double)c.B * c.H * c.W * 8.0 >= kTooBig) return UAPS_ERANGE;
    Plan p;
    const int rc = make_plan(c.H, c.W, c.n_classes, reach, c.band_rows, p);
    if (rc) return rc;

    MorphArgs a;
    memset(&a, 0, sizeof a);
    a.B = c.B; a.H = c.H; a.W = c.W; a.nw = (c.W + 63) / 64;
    a.n = c.n_classes; a.G = p.G;
    a.band = p.band; a.reach = reach; a.R = p.band + 2 * reach;
    a.tw = p.tw; a.sw = p.sw; a.hx = p.hx; a.ntx = p.ntx; a.nby = (c.H + p.band - 1) / p.band;
    a.n_steps = c.n_steps;
    for (int s = 0; s < c.n_steps; ++s) {
        const int r = c.radius[s];
        a.op[s] = c.op[s]; a.radius[s] = r;
        for (int d = 0; d <= r; ++d) {
            int w = r;                          // square
            if (c.footprint[s] == UAPS_MORPH_CROSS) w = r - d;
            if (c.footprint[s] == UAPS_MORPH_DISK) {
                w = 0;
                while ((w + 1) * (w + 1) + d * d <= r * r) ++w;
            }
            a.hw[s] |= (u64)w << (4 * d);
        }
    }
    for (int k = 0; k < c.n_classes; ++k) a.cls[k] = c.classes[k];
    for (int k = 1; k < c.n_classes; ++k)       // ascending: the smallest class claims first
        for (int j = k; j > 0 && a.cls[j - 1] > a.cls[j]; --j) { const long long v = a.cls[j]; a.cls[j] = a.cls[j - 1]; a.cls[j - 1] = v; }
    a.bg = c.background;
    a.mask = (const long long*)c.mask; a.out = (long long*)c.out;
    const size_t lds_bytes = (size_t)(a.n + 2 + 2 * a.G) * a.R * a.sw * 8;     // <= 64 KiB by make_plan
    const long blocks = (long)c.B * a.nby * a.ntx;                            // <= B * H * W < 2^28
    uaps::account_bytes(16.0 * c.B * c.H * c.W);
    UAPS_LAUNCH_MAIN(morph_chain_kernel, dim3((unsigned)blocks), dim3(kThreads), lds_bytes, (hipStream_t)c.stream, a);
    return (int)hipGetLastError();
}
