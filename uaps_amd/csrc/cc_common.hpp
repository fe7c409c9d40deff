// Connected-component labelling shared by instances.hip (uaps_label_instances) and components.hip (uaps_components): the union-find
// device functions and the three labelling passes -- tile-local in LDS, seam merge, flatten + area -- over Q planes of H x W pixels.
//
// What differs between the users is the POLICY, a small struct passed by value inside CcArgs:
//   image(q)     which image of the mask plane q looks at (q itself where a plane is an image; q / n for n virtual planes an image)
//   fg(v, q)     whether a pixel of value v forms components in plane q at all
//   key(v, q)    two neighbouring foreground pixels belong together where their keys are equal
// and the MARK of cc_flatten_area: which pixels raise bit 31 of their component's area word (NoMark: none; BorderMark: those on the
// image border; a user's own: hysteresis.hip marks the seeds of its code map).
//
// Every parent word holds the plane-local index of an earlier or equal pixel of the same component (-1: not foreground), only ever
// decreases, and a walk ends at the word that names itself: the component's first pixel in raster order.  No workgroup waits for
// another inside a launch (no flags, no spin loops): every union loop ends by the monotone decrease of the parent words alone.
//
// Builds on call_common.hpp alone (kThreads, kWaves of the enclosing namespace): nothing of the loss scaffold comes with this header.
#pragma once
#include "call_common.hpp"

namespace uaps {
namespace cc {
constexpr int kTW = 16, kTH = 16, kTile = kTW * kTH, kPer = kTile / kThreads;   // pixels of a tile per lane
constexpr unsigned kBorderBit = 0x80000000u;                                    // the mark bit of an area word (H * W < 2^31 leaves it free)
constexpr unsigned kAreaMask = 0x7fffffffu;

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_wg(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// parent[x] <= x always and only ever decreases: a walk strictly descends and ends at a word that names itself
template <bool GLOBAL>
__device__ __forceinline__ int uf_find(const int* par, int a) {
    for (;;) {
        const int p = GLOBAL ? ld_agent(par + a) : ld_wg(par + a);
        if (p == a) return a;
        a = p;
    }
}

// parent words are final when the flatten pass runs (the launch boundary made them visible): plain loads
__device__ __forceinline__ int uf_find_plain(const int* par, int a) {
    for (;;) {
        const int p = par[a];
        if (p == a) return a;
        a = p;
    }
}

// joins the trees of a and b: the larger root is lowered onto the smaller one.  A failed atomicMin means somebody else lowered that
// word in the meantime: go on from what it holds now, which is smaller -- nothing here waits for another lane's progress.
template <bool GLOBAL>
__device__ __forceinline__ void uf_union(int* par, int a, int b) {
    for (;;) {
        a = uf_find<GLOBAL>(par, a);
        b = uf_find<GLOBAL>(par, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + b, a);
        if (old == b) return;
        b = old;
    }
}

// components of equal values; pixels of `bg` form none when has_bg
struct SameValuePolicy {
    int has_bg;
    long long bg;
    __device__ __forceinline__ int image(int q) const { return q; }
    __device__ __forceinline__ bool fg(long long v, int) const { return !(has_bg && v == bg); }
    __device__ __forceinline__ long long key(long long v, int) const { return v; }
};

template <typename Policy>
struct CcArgs {
    int Q, H, W, ntx, nty, conn8;       // Q planes
    const long long* mask;              // [images][H][W]
    int* parent;                        // [Q][H][W]
    int* area;                          // [Q][H][W]
    Policy pol;
};

// One workgroup per (plane, 16 x 16 tile): union-find with atomicMin over the backward neighbours of every pixel in LDS, then every
// pixel's parent := the plane-local index of its tile-local root (tile-local raster order and image raster order agree inside a
// tile).  Plain stores; the area word of every pixel is zeroed on the way.
template <typename Policy>
__device__ __forceinline__ void cc_tile_label(const CcArgs<Policy>& a, long long* cls, int* lab) {
    const long tiles = (long)a.ntx * a.nty;
    const long blk = blockIdx.x;
    const int q = (int)(blk / tiles);
    const int t = (int)(blk - (long)q * tiles);
    const int ty = t / a.ntx, tx = t - ty * a.ntx;
    const long HW = (long)a.H * a.W;
    const long long* m = a.mask + (long)a.pol.image(q) * HW;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int li = threadIdx.x + k * kThreads, ly = li / kTW, lx = li % kTW;
        const int y = ty * kTH + ly, x = tx * kTW + lx;
        long long c = 0;
        bool fg = false;
        if (y < a.H && x < a.W) {
            const long long v = m[(long)y * a.W + x];
            fg = a.pol.fg(v, q);
            c = a.pol.key(v, q);
        }
        cls[li] = c;
        lab[li] = fg ? li : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int li = threadIdx.x + k * kThreads, ly = li / kTW, lx = li % kTW;
        if (lab[li] < 0) continue;             // (-1 never changes; a foreground word stays >= 0)
        const long long c = cls[li];
        if (lx > 0 && lab[li - 1] >= 0 && cls[li - 1] == c) uf_union<false>(lab, li, li - 1);
        if (ly > 0) {
            if (lab[li - kTW] >= 0 && cls[li - kTW] == c) uf_union<false>(lab, li, li - kTW);
            if (a.conn8) {
                if (lx > 0 && lab[li - kTW - 1] >= 0 && cls[li - kTW - 1] == c) uf_union<false>(lab, li, li - kTW - 1);
                if (lx < kTW - 1 && lab[li - kTW + 1] >= 0 && cls[li - kTW + 1] == c) uf_union<false>(lab, li, li - kTW + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int li = threadIdx.x + k * kThreads, ly = li / kTW, lx = li % kTW;
        const int y = ty * kTH + ly, x = tx * kTW + lx;
        if (y >= a.H || x >= a.W) continue;
        int out = -1;
        if (lab[li] >= 0) {
            const int r = uf_find<false>(lab, li);
            out = (ty * kTH + r / kTW) * a.W + tx * kTW + r % kTW;
        }
        const long n = (long)q * HW + (long)y * a.W + x;
        a.parent[n] = out;
        a.area[n] = 0;
    }
}

// per plane: (nty - 1) * W pixels on the first row of a tile row, then (ntx - 1) * H pixels on the first column of a tile column.
// One lane per seam pixel and its up to three neighbours across the seam.  Every parent word is read with relaxed agent-scope atomic
// loads and lowered with atomicMin.  A stale read is an older parent, still an ancestor in the same component, so it costs
// iterations, never correctness.
template <typename Policy>
__device__ __forceinline__ void cc_seam_merge(const CcArgs<Policy>& a) {
    const long HW = (long)a.H * a.W;
    const long nH = (long)(a.nty - 1) * a.W, per = nH + (long)(a.ntx - 1) * a.H, total = (long)a.Q * per;
    for (long g = (long)blockIdx.x * kThreads + threadIdx.x; g < total; g += (long)gridDim.x * kThreads) {
        const int q = (int)(g / per);
        long j = g - (long)q * per;
        const long long* m = a.mask + (long)a.pol.image(q) * HW;
        int* par = a.parent + (long)q * HW;
        int p, pos, len, along, across;         // the pixel, its place on the seam, and the index steps along and across the seam
        if (j < nH) {                           // the three neighbours in the row above
            const int y = ((int)(j / a.W) + 1) * kTH, x = (int)(j % a.W);
            p = y * a.W + x; pos = x; len = a.W; along = 1; across = a.W;
        } else {                                // the three neighbours in the column to the left
            j -= nH;
            const int x = ((int)(j / a.H) + 1) * kTW, y = (int)(j % a.H);
            p = y * a.W + x; pos = y; len = a.H; along = a.W; across = 1;
        }
        const long long v = m[p];
        if (!a.pol.fg(v, q)) continue;
        const long long c = a.pol.key(v, q);
        auto same = [&](int o) { const long long u = m[o]; return a.pol.fg(u, q) && a.pol.key(u, q) == c; };
        // Only the joins the tile pass does not already imply.  Neighbours ALONG the seam inside one tile (kTW == kTH) were joined
        // there, on both sides of the seam.  So the join straight across is left to the previous seam pixel where that one and its
        // opposite belong to this pixel too -- down a run, to the run's first pixel in the tile, which does it -- and a diagonal join
        // is implied where the straight one of this pixel, or of the seam neighbour beside that diagonal, exists.  The roots do not
        // depend on which joins of a component are made: a solid region sends one atomicMin a tile edge, not sixteen.
        const bool has_prev = pos > 0, has_next = pos < len - 1;
        const bool in_prev = pos % kTW != 0, in_next = has_next && (pos + 1) % kTW != 0;     // the seam neighbour lies in this tile
        const bool s_opp = same(p - across);
        const bool s_opp_prev = has_prev && same(p - across - along), s_opp_next = has_next && same(p - across + along);
        const bool s_prev = in_prev && same(p - along), s_next = in_next && same(p + along);
        if (s_opp && !(s_prev && s_opp_prev)) uf_union<true>(par, p, p - across);
        if (a.conn8) {
            if (s_opp_prev && !(in_prev && (s_opp || s_prev))) uf_union<true>(par, p, p - across - along);
            if (s_opp_next && !(in_next && (s_opp || s_next))) uf_union<true>(par, p, p - across + along);
        }
    }
}

// the last lane of the run of lanes that lane `lane` belongs to; heads = ballot of the runs' first lanes (bit 0 set)
__device__ __forceinline__ int run_end(unsigned long long heads, int lane) {
    const unsigned long long above = lane < 63 ? heads >> (lane + 1) : 0ull;
    return above ? lane + __builtin_ctzll(above) : 63;
}

// A wave walks kSpan consecutive groups of 64 pixels and carries what the groups contributed to ONE key (`pending`, wave-uniform) from
// group to group: a component that fills rows sends one atomic per kSpan * 64 pixels instead of one per 64.
constexpr int kSpan = 16;
inline int span_grid(long N) { return (int)((N + (long)kThreads * kSpan - 1) / ((long)kThreads * kSpan)); }

// The mark policy of cc_flatten_area: mark(n, i) of a foreground pixel -- n its index over all planes, i its plane-local index --
// says whether the pixel raises kBorderBit of its component's area word.  kOn == false: no flag is formed at all.
struct NoMark {
    static constexpr bool kOn = false;
    __device__ __forceinline__ bool operator()(long, long) const { return false; }
};
// the pixels of row 0, row H - 1, column 0 and column W - 1
struct BorderMark {
    static constexpr bool kOn = true;
    int H, W;
    __device__ __forceinline__ bool operator()(long, long i) const {
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        return y == 0 || y == H - 1 || x == 0 || x == W - 1;
    }
};

template <bool FLAG>
__device__ __forceinline__ void cc_send(int* word, int n, bool border) {
    atomicAdd(word, n);
    if (FLAG && border) atomicOr(word, (int)kBorderBit);
}

// parent -> root (the component's smallest pixel index = its first pixel), stored into `roots`, and the areas: integer atomicAdds
// onto the roots' area words.  Per group of 64 pixels, all lanes of the group's LEADING root -- that of its first foreground lane,
// wherever in the group they sit -- are counted by one ballot and carried on by the wave over its kSpan groups while the leading root
// stays the same; the other roots of the group send one atomicAdd per run of equal roots.  So a component that fills rows, and
// equally one that is porous (class noise; the complement of a class in hole filling), costs one atomic per kSpan * 64 pixels and
// not one per run: thousands of adds to ONE word serialise at the memory side.  Mark::kOn: what is sent for pixels among which one is
// marked also raises kBorderBit of that word, once per send -- on BOTH paths, the wave-carried leading root and the per-run adds of
// the other roots: a mark may sit on any pixel of a component, not only on the border.  N = Q * HW pixels; HW = H * W.
// `roots` may be `parent` itself (components.hip): a word is then overwritten by its own lane alone, with its root, while other
// lanes may still walk through it -- they read the old parent or the root, and either is an ancestor in the same component.
template <typename Mark>
__device__ __forceinline__ void cc_flatten_area(const int* parent, int* roots, int* area, long HW, long N, const Mark mark) {
    constexpr bool FLAG = Mark::kOn;
    const int lane = threadIdx.x & 63;
    const long w0 = ((long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * (kSpan * 64);
    long pend_b = -1;
    int pend_r = -1, pend_n = 0;
    bool pend_f = false;
    for (int it = 0; it < kSpan; ++it) {
        const long base = w0 + (long)it * 64;
        if (base >= N) break;                  // (wave-uniform)
        const long n = base + lane;
        const bool valid = n < N;
        int r = -2;
        long b = 0, i = 0;
        bool edge = false;
        if (valid) {
            b = n / HW; i = n - b * HW;
            const int* par = parent + b * HW;
            r = par[i];
            if (r >= 0) r = uf_find_plain(par, r);
            roots[n] = r;
            if (FLAG && r >= 0) edge = mark(n, i);
        }
        const int prev = __shfl_up(r, 1, 64);
        const bool head = lane == 0 || prev != r || i == 0;
        const unsigned long long heads = __ballot(head);
        const unsigned long long edges = FLAG ? __ballot(edge) : 0ull;
        const unsigned long long fgm = __ballot(r >= 0);
        if (fgm == 0ull) continue;             // (wave-uniform; what is pending stays pending)
        const int first = __builtin_ctzll(fgm);
        const int rl = __shfl(r, first, 64);
        const long bl = __shfl(b, first, 64);
        const bool lead = r == rl && b == bl;
        const unsigned long long leads = __ballot(lead);
        if (!(pend_n > 0 && pend_r == rl && pend_b == bl)) {
            if (pend_n > 0 && lane == 0) cc_send<FLAG>(area + pend_b * HW + pend_r, pend_n, pend_f);
            pend_b = bl; pend_r = rl; pend_n = 0; pend_f = false;
        }
        pend_n += __popcll(leads);
        pend_f = pend_f || (edges & leads) != 0ull;
        if (head && r >= 0 && !lead) {         // (a run holds one root: all of its lanes lead or none does)
            const int len = run_end(heads, lane) - lane + 1;
            const unsigned long long in_run = (len == 64 ? ~0ull : (1ull << len) - 1ull) << lane;
            cc_send<FLAG>(area + b * HW + r, len, (edges & in_run) != 0ull);
        }
    }
    if (pend_n > 0 && lane == 0) cc_send<FLAG>(area + pend_b * HW + pend_r, pend_n, pend_f);
}

}  // namespace cc
}  // namespace uaps
