// Tiled (sliding-window) full-resolution inference for gfx950 (include/uaps_hip.h, uaps_tile_origins / uaps_tile_cut / uaps_tile_fold):
// an image of any size is cut into overlapping tiles of the size the network runs at, and the tiles' probability maps are blended
// under a separable window.  Two kernels stand around the network's forwards, as in tta.hip:
//   tile_cut_kernel    the input side of ONE chunk of tiles: x [B,Cin,H,W] -> [g1-g0,Cin,th,tw], a copy (mirrored index where an image
//                      extent is below the tile's)
//   tile_fold_kernel   the output side of ALL tiles, gather form: a lane owns V consecutive output pixels and keeps their C weighted
//                      sums and the weight sum in registers; it finds the (at most 3 x 3) covering tiles from the origin formula,
//                      visits them in ascending (iy, ix) order, takes the softmax of each tile's logits at the pixel, weights it by
//                      wy[r] * wx[c] and adds; at the end it divides and writes the mean, its arg-max and the confidence.  No LDS, no
//                      atomics, no cross-lane sums, no table in memory: two runs, and two chunkings of the same tiles, give the same bits.
// Geometry per axis (extent n, tile t, overlap o <= t / 2, stride s = t - o): cnt = 1 and last = 0 when n <= t, else
// cnt = ceil((n - t) / s) + 1 and last = n - t; tile i starts at i * s for i < cnt - 1 and at `last` for i = cnt - 1.  Pixel p lies in
// the regular tiles k - 1 and k, k = p / s (where those exist and reach p: t <= 2 s, so k - 2 never does), and in the last tile when
// p >= last: three candidates, already in ascending order.
#include "loss_common.hpp"               // uaps::pixel (the softmax of a pixel's logits), UAPS_BY_C, UAPS_LAUNCH_V
#include "rn_math.hpp"

namespace {
using uaps::kThreads; using uaps::kTooBig; using uaps::grid_for; using uaps::al16;
constexpr int kMaxChunks = UAPS_TILE_MAX_CHUNKS, kMaxMaps = UAPS_TILE_MAX_MAPS;
constexpr int kMaxBlocks = 1 << 20;      // every tensor is below 2 GiB: a grid never needs more; the lanes stride over the rest anyway

struct Axis { int n, t, s, cnt, last; };

inline Axis axis_of(int n, int t, int o) {
    Axis a;
    a.n = n; a.t = t; a.s = t - o;
    a.cnt = n <= t ? 1 : (n - t + a.s - 1) / a.s + 1;
    a.last = n <= t ? 0 : n - t;
    return a;
}

__device__ __forceinline__ int origin(const Axis& a, int i) { return i == a.cnt - 1 ? a.last : i * a.s; }

// the source of tile position i of an axis of n < t pixels: mirrored, the edge not repeated
__device__ __forceinline__ int mirror(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1), j = i % period;
    return j < n ? j : period - j;
}

// the tiles of one axis that hold pixel p, ascending: idx[j] (-1: none) and p's position loc[j] inside tile idx[j]
__device__ __forceinline__ void cover(const Axis& a, int p, int (&idx)[3], int (&loc)[3]) {
    const int k = p / a.s;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int kk = k - 1 + j, r = p - kk * a.s;          // r >= 0: kk <= k
        idx[j] = (kk >= 0 && kk <= a.cnt - 2 && r < a.t) ? kk : -1;
        loc[j] = r;
    }
    idx[2] = p >= a.last ? a.cnt - 1 : -1;
    loc[2] = p - a.last;
}

struct CutArgs {
    int Cin, H, W, nx, T, g0;
    long n;                              // elements this launch writes
    Axis ay, ax;
    const float* x; float* out;
};

// one lane per element of the chunk
__global__ __launch_bounds__(kThreads) void tile_cut_kernel(CutArgs a) {
    const long tpix = (long)a.ay.t * a.ax.t, per = (long)a.Cin * tpix;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (long)gridDim.x * kThreads) {
        const long k = i / per, rem = i - k * per;
        const int c = (int)(rem / tpix), pix = (int)(rem - (long)c * tpix);
        const int r = pix / a.ax.t, col = pix - r * a.ax.t;
        const int g = a.g0 + (int)k, b = g / a.T, q = g - b * a.T, iy = q / a.nx, ix = q - iy * a.nx;
        int y = origin(a.ay, iy) + r, x = origin(a.ax, ix) + col;
        if (a.H < a.ay.t) y = mirror(y, a.H);                // one tile at origin 0; otherwise no tile leaves the image
        if (a.W < a.ax.t) x = mirror(x, a.W);
        a.out[i] = a.x[(((long)b * a.Cin + c) * a.H + y) * a.W + x];
    }
}

struct FoldArgs {
    int B, H, W, nx, T, n_chunks, tpc, n_maps;
    Axis ay, ax;
    const float* wy; const float* wx;
    const float* z[kMaxChunks];
    const float* m[kMaxMaps][kMaxChunks];
    float* mo[kMaxMaps];
    float* probs; long long* mask; float* conf;
};

// chunk and position inside it of tile g
__device__ __forceinline__ void locate(const FoldArgs& a, int g, int& ch, int& k) {
    ch = a.n_chunks > 1 ? g / a.tpc : 0;
    k = g - ch * a.tpc;
}

// V = 4 needs W % 4 == 0 (a group never straddles two rows) and 16-byte aligned outputs.  C = 0: the maps alone.
template <int C, int V>
__global__ __launch_bounds__(kThreads, 2) void tile_fold_kernel(FoldArgs a) {
    constexpr int CA = C > 0 ? C : 1;
    const long HW = (long)a.H * a.W, groups = (long)a.B * HW / V, tpix = (long)a.ay.t * a.ax.t;
    for (long grp = (long)blockIdx.x * kThreads + threadIdx.x; grp < groups; grp += (long)gridDim.x * kThreads) {
        const long n = grp * V;
        const int b = (int)(n / HW);
        const long pix = n - (long)b * HW;
        const int y = (int)(pix / a.W), x = (int)(pix - (long)y * a.W);
        int iy[3], ry[3], ix[V][3], rx[V][3];
        cover(a.ay, y, iy, ry);
#pragma unroll
        for (int v = 0; v < V; ++v) cover(a.ax, x + v, ix[v], rx[v]);
        float acc[CA][V], ws[V], ma[kMaxMaps][V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            ws[v] = 0.f;
#pragma unroll
            for (int c = 0; c < CA; ++c) acc[c][v] = 0.f;
#pragma unroll
            for (int m = 0; m < kMaxMaps; ++m) ma[m][v] = 0.f;
        }
#pragma unroll
        for (int jy = 0; jy < 3; ++jy) {
            if (iy[jy] < 0) continue;
            const float wyv = a.wy[ry[jy]];
            const int row = b * a.T + iy[jy] * a.nx;
#pragma unroll
            for (int jx = 0; jx < 3; ++jx) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if (ix[v][jx] < 0) continue;
                    int ch, k;
                    locate(a, row + ix[v][jx], ch, k);
                    const long off = (long)k * tpix + (long)ry[jy] * a.ax.t + rx[v][jx];      // in a one-plane tensor of the chunk
                    // the weight is rounded on its own and every weighted add is ONE fused multiply-add, written out: left to the
                    // compiler's contraction the two store forms fused differently and disagreed in the last bit
                    const float w = uaps::mul_rn(wyv, a.wx[rx[v][jx]]);
                    ws[v] += w;
                    if constexpr (C > 0) {
                        float z[C][1], mx[1], lse[1];
                        uaps::pixel::load_logits<C, 1>(a.z[ch] + (long)k * (C - 1) * tpix + off, tpix, z);
                        uaps::pixel::softmax_inplace<C, 1>(z, mx, lse);
#pragma unroll
                        for (int c = 0; c < C; ++c) acc[c][v] = __builtin_fmaf(w, z[c][0], acc[c][v]);
                    }
#pragma unroll
                    for (int m = 0; m < kMaxMaps; ++m)
                        if (m < a.n_maps) ma[m][v] = __builtin_fmaf(w, a.m[m][ch][off], ma[m][v]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < kMaxMaps; ++m)
            if (m < a.n_maps) {
                float t[1][V];
#pragma unroll
                for (int v = 0; v < V; ++v) t[0][v] = ma[m][v] / ws[v];
                uaps::pixel::store_planes<1, V>(a.mo[m] + n, 0, t);
            }
        if constexpr (C > 0) {
#pragma unroll
            for (int v = 0; v < V; ++v)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c][v] = acc[c][v] / ws[v];
            if (a.probs) uaps::pixel::store_planes<C, V>(a.probs + (long)b * C * HW + pix, HW, acc);
            if (a.mask || a.conf) {
                int am[V];
                uaps::pixel::argmax_logits<C, V>(acc, am);              // of the MEAN: the mask is the arg-max of what probs holds
                if (a.mask) {
                    if constexpr (V == 4) {
                        longlong2* mk = reinterpret_cast<longlong2*>(a.mask + n);
                        mk[0] = make_longlong2(am[0], am[1]);
                        mk[1] = make_longlong2(am[2], am[3]);
                    } else {
                        a.mask[n] = am[0];
                    }
                }
                if (a.conf) {
                    float cf[1][V];
#pragma unroll
                    for (int v = 0; v < V; ++v) cf[0][v] = uaps::pixel::pick<C, V>(acc, v, am[v]);
                    uaps::pixel::store_planes<1, V>(a.conf + n, 0, cf);
                }
            }
        }
    }
}

inline bool too_big(double elems, double bytes_each) { return elems * bytes_each >= kTooBig; }

template <int C>
int launch_fold(const FoldArgs& a, bool vec, hipStream_t st) {
    const long groups = (long)a.B * a.H * a.W / (vec ? 4 : 1);
    const int grid = grid_for(groups, kMaxBlocks);
    UAPS_LAUNCH_V(vec, tile_fold_kernel, C, grid, st, a);
    return (int)hipGetLastError();
}

// UAPS_EINVAL / UAPS_ERANGE / 0 for the geometry both entry points share
int check_geometry(int H, int W, int th, int tw, int oy, int ox) {
    if (H <= 0 || W <= 0 || th <= 0 || tw <= 0 || oy < 0 || ox < 0) return UAPS_EINVAL;
    if (oy > th / 2 || ox > tw / 2) return UAPS_ERANGE;
    return 0;
}
}  // namespace

extern "C" int uaps_tile_origins(int n, int tile, int overlap, int* count, int* origins, int cap) {
    if (!count || n < 1 || tile < 1 || overlap < 0 || cap < 0) return UAPS_EINVAL;
    if (overlap > tile / 2) return UAPS_ERANGE;
    const Axis a = axis_of(n, tile, overlap);
    *count = a.cnt;
    if (origins)
        for (int i = 0; i < a.cnt && i < cap; ++i) origins[i] = i == a.cnt - 1 ? a.last : i * a.s;
    return 0;
}

extern "C" int uaps_tile_cut(const uaps_tile_cut_call* call) {
    uaps_tile_cut_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.x || !c.out || c.B <= 0 || c.Cin <= 0) return UAPS_EINVAL;
    if (const int rc = check_geometry(c.H, c.W, c.th, c.tw, c.oy, c.ox)) return rc;
    if (too_big((double)c.B * c.Cin * c.H * c.W, 4.0)) return UAPS_ERANGE;
    const Axis ay = axis_of(c.H, c.th, c.oy), ax = axis_of(c.W, c.tw, c.ox);       // cnt <= n: B * T <= B * H * W < 2^29
    const long T = (long)ay.cnt * ax.cnt, tiles = (long)c.B * T;
    if (c.g0 < 0 || c.g0 >= c.g1 || c.g1 > tiles) return UAPS_EINVAL;
    const double elems = (double)(c.g1 - c.g0) * c.Cin * c.th * c.tw;
    if (too_big(elems, 4.0)) return UAPS_ERANGE;
    CutArgs a;
    a.Cin = c.Cin; a.H = c.H; a.W = c.W; a.nx = ax.cnt; a.T = (int)T; a.g0 = c.g0;
    a.n = (long)elems;
    a.ay = ay; a.ax = ax; a.x = c.x; a.out = c.out;
    uaps::account_bytes(8.0 * elems);        // every tile element read once and written once
    UAPS_LAUNCH_MAIN(tile_cut_kernel, dim3(grid_for(a.n, kMaxBlocks)), dim3(kThreads), 0, (hipStream_t)c.stream, a);
    return (int)hipGetLastError();
}

extern "C" int uaps_tile_fold(const uaps_tile_fold_call* call) {
    uaps_tile_fold_call c;
    if (uaps::read_call(call, c)) return UAPS_EINVAL;
    if (!c.wy || !c.wx || c.B <= 0 || c.C < 0 || c.n_maps < 0 || c.n_chunks <= 0 || c.tiles_per_chunk <= 0) return UAPS_EINVAL;
    const bool any_class_out = c.probs || c.mask || c.conf;
    if ((c.C == 0 && any_class_out) || (!any_class_out && c.n_maps == 0) || (c.C > 0 && !any_class_out)) return UAPS_EINVAL;
    if (const int rc = check_geometry(c.H, c.W, c.th, c.tw, c.oy, c.ox)) return rc;
    if (c.C == 1 || c.C > UAPS_MAX_CLASSES || c.n_chunks > kMaxChunks || c.n_maps > kMaxMaps) return UAPS_ERANGE;
    for (int k = 0; k < c.n_chunks; ++k) {
        if (c.C > 0 && !c.logits[k]) return UAPS_EINVAL;
        for (int m = 0; m < c.n_maps; ++m)
            if (!c.maps[m][k]) return UAPS_EINVAL;
    }
    for (int m = 0; m < c.n_maps; ++m)
        if (!c.map_out[m]) return UAPS_EINVAL;
    const double pixels = (double)c.B * c.H * c.W;
    // the outputs the call writes: a NULL one is no tensor.  One of them exists, so B * H * W < 2^29 from here on.
    if ((c.probs && too_big(pixels * c.C, 4.0)) || (c.mask && too_big(pixels, 8.0)) || ((c.conf || c.n_maps) && too_big(pixels, 4.0)))
        return UAPS_ERANGE;
    const Axis ay = axis_of(c.H, c.th, c.oy), ax = axis_of(c.W, c.tw, c.ox);
    const long T = (long)ay.cnt * ax.cnt, tiles = (long)c.B * T;                   // cnt <= n: tiles <= B * H * W
    if ((long)(c.n_chunks - 1) * c.tiles_per_chunk >= tiles || (long)c.n_chunks * c.tiles_per_chunk < tiles) return UAPS_EINVAL;
    const double chunk_tiles = (double)(c.tiles_per_chunk < tiles ? c.tiles_per_chunk : tiles), tpix = (double)c.th * c.tw;
    if (too_big(chunk_tiles * (c.C > 0 ? c.C : 1) * tpix, 4.0)) return UAPS_ERANGE;
    FoldArgs a;
    memset(&a, 0, sizeof a);
    a.B = c.B; a.H = c.H; a.W = c.W; a.nx = ax.cnt; a.T = (int)T; a.n_chunks = c.n_chunks; a.tpc = c.tiles_per_chunk; a.n_maps = c.n_maps;
    a.ay = ay; a.ax = ax; a.wy = c.wy; a.wx = c.wx;
    bool vec = c.W % 4 == 0 && al16(c.probs) && al16(c.mask) && al16(c.conf);
    for (int k = 0; k < c.n_chunks; ++k) {
        a.z[k] = c.logits[k];
        for (int m = 0; m < c.n_maps; ++m) a.m[m][k] = c.maps[m][k];
    }
    for (int m = 0; m < c.n_maps; ++m) { a.mo[m] = c.map_out[m]; vec = vec && al16(c.map_out[m]); }
    a.probs = c.probs; a.mask = (long long*)c.mask; a.conf = c.conf;
    // every tile element read once (mirror padding included: an upper bound where an image is smaller than the tile), every output once
    uaps::account_bytes(4.0 * ((double)tiles * tpix * (c.C + c.n_maps) + (double)c.th + c.tw) +
                        pixels * ((c.probs ? 4.0 * c.C : 0.0) + (c.mask ? 8.0 : 0.0) + (c.conf ? 4.0 : 0.0) + 4.0 * c.n_maps));
    hipStream_t st = (hipStream_t)c.stream;
    if (c.C == 0) return launch_fold<0>(a, vec, st);
#define UAPS_TILE_FOLD(Cc) launch_fold<Cc>(a, vec, st)
    UAPS_BY_C(c.C, UAPS_TILE_FOLD);
#undef UAPS_TILE_FOLD
}
