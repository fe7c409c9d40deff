"""The reference of the convex-hull tests (tests/test_hull_host.py, tests/test_gpu_hull.py): brute force, one label at a time.
The four corners of every pixel of a label as a point set, Andrew's monotone chain over the SORTED points on Python integers, the
farthest pair over all vertex pairs, and both edge minimisations over all (edge, vertex) pairs with fractions.Fraction.  It shares
nothing with the package's numpy path (row extents and two lattice-line chains) or with the kernels.  Also the case table both
test files run."""
import functools
from fractions import Fraction

import numpy as np

COLUMNS = ("nv", "area2", "fmax_sq", "f_y0", "f_x0", "f_y1", "f_x1", "w_ey", "w_ex", "w_c",
           "r_y", "r_x", "r_ey", "r_ex", "r_dmin", "r_dmax", "r_c")
MS = (1, 3, 256, 257)           # the kernels have one form for every M; 256 / 257 are the sizes at which shapes.hip changes its own
THREADS = 256                   # of a workgroup of csrc/hull.hip: edges and vertices are dealt to threads with this stride


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def vertices(ys, xs):
    """The strict hull vertices (x, y) of the pixel squares, in hull order: from the smallest (y, x) along the top edge towards +x."""
    ys, xs = np.asarray(ys, dtype=np.int64), np.asarray(xs, dtype=np.int64)
    corners = np.concatenate([np.stack([xs + dx, ys + dy], axis=1) for dy in (0, 1) for dx in (0, 1)])
    pts = sorted(set(map(tuple, corners.tolist())))
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = lower[:-1] + upper[:-1]              # counter-clockwise with y upwards = clockwise on the screen
    s = min(range(len(hull)), key=lambda i: (hull[i][1], hull[i][0]))
    return hull[s:] + hull[:s]


def edge_values(V):
    """Per edge i of the vertex list: (ex, ey, C, dmin, dmax), C and the extremes of d by a loop over all vertices."""
    out = []
    n = len(V)
    for i in range(n):
        vx, vy = V[i]
        ex, ey = V[(i + 1) % n][0] - vx, V[(i + 1) % n][1] - vy
        cs = [ex * (py - vy) - ey * (px - vx) for px, py in V]
        ds = [ex * (px - vx) + ey * (py - vy) for px, py in V]
        assert min(cs) == 0
        out.append((ex, ey, max(cs), min(ds), max(ds)))
    return out


def row_of(V):
    """The 17 columns of a vertex list, every rule by brute force."""
    n = len(V)
    area2 = sum(V[i][0] * V[(i + 1) % n][1] - V[(i + 1) % n][0] * V[i][1] for i in range(n))
    pairs = []
    for i in range(n):
        for j in range(i + 1, n):
            p, q = sorted(((V[i][1], V[i][0]), (V[j][1], V[j][0])))
            pairs.append((-((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2), p[0], p[1], q[0], q[1]))
    far = min(pairs)
    ev = edge_values(V)
    w = min(range(n), key=lambda i: (Fraction(ev[i][2] ** 2, ev[i][0] ** 2 + ev[i][1] ** 2), i))
    r = min(range(n), key=lambda i: (Fraction((ev[i][4] - ev[i][3]) * ev[i][2], ev[i][0] ** 2 + ev[i][1] ** 2), i))
    return [n, area2, -far[0], far[1], far[2], far[3], far[4], ev[w][1], ev[w][0], ev[w][2],
            V[r][1], V[r][0], ev[r][1], ev[r][0], ev[r][3], ev[r][4], ev[r][2]]


def table(labels, M):
    """labels int32 [B,H,W] -> int64 [B,M,17]; labels outside [1, M] have no row."""
    B = labels.shape[0]
    out = np.zeros((B, M, 17), dtype=np.int64)
    for b in range(B):
        y, x = np.nonzero((labels[b] >= 1) & (labels[b] <= M))
        k = labels[b][y, x]
        for kk in np.unique(k):
            out[b, kk - 1] = row_of(vertices(y[k == kk], x[k == kk]))
    return out


def instance_table(labels, M):
    """(count int32 [B], table int64 [B,M,9]) as label_instances lays them out: cls (0 here), area, y0, x0, y1, x1 (exclusive)."""
    B = labels.shape[0]
    tab = np.zeros((B, M, 9), dtype=np.int64)
    count = np.zeros(B, dtype=np.int32)
    for b in range(B):
        y, x = np.nonzero((labels[b] >= 1) & (labels[b] <= M))
        k = labels[b][y, x]
        for kk in np.unique(k):
            s = k == kk
            tab[b, kk - 1, 1:6] = s.sum(), y[s].min(), x[s].min(), y[s].max() + 1, x[s].max() + 1
        count[b] = len(np.unique(k))
    return count, tab


# ------------------------------------------------------------------------------------------------ fillings: label maps [B,H,W] int32
def _one(B, H, W):
    m = np.zeros((B, H, W), dtype=np.int32)
    m[:, H - 1, W // 2] = 1
    return m


def _full(B, H, W):
    return np.ones((B, H, W), dtype=np.int32)


def _noise3(B, H, W):
    return np.random.default_rng(7).integers(0, 4, (B, H, W)).astype(np.int32)


def _checker4(B, H, W):
    """Blocks of 2 x 2 pixels (cut at the frame), every other one a label of its own, numbered in raster order from 1: sixteen
    labels inside one group of 64 lanes, and far more labels than rows."""
    y, x = np.mgrid[0:H, 0:W]
    by, bx = y // 2, x // 2
    on = (by + bx) % 2 == 0
    idx = by * ((W + 1) // 2) + bx
    rank = np.cumsum(np.bincount(idx[on].ravel(), minlength=idx.max() + 1) > 0)
    m = np.where(on, rank[idx], 0).astype(np.int32)
    return np.repeat(m[None], B, axis=0)


def _rings(B, H, W):
    """Label 1 the frame's rim, label 2 a rim inside it, label 3 a blob in the middle: 2 and 3 lie inside the hull of 1."""
    m = np.zeros((B, H, W), dtype=np.int32)
    m[:, [0, -1], :] = 1
    m[:, :, [0, -1]] = 1
    if H > 4 and W > 4:
        m[:, 2, 2:W - 2] = m[:, H - 3, 2:W - 2] = 2
        m[:, 2:H - 2, 2] = m[:, 2:H - 2, W - 3] = 2
    if H > 8 and W > 8:
        m[:, H // 2 - 1:H // 2 + 1, W // 2 - 2:W // 2 + 2] = 3
    return m


def _diagonal(B, H, W):
    """One pixel a row (or a column, on a wide frame), spread over the whole frame: a one-pixel-wide diagonal of label 1."""
    m = np.zeros((B, H, W), dtype=np.int32)
    n = max(H, W)
    i = np.arange(n)
    m[:, i * H // n, i * W // n] = 1
    return m


def _anti(B, H, W):
    return _diagonal(B, H, W)[:, :, ::-1].copy()


def _far(B, H, W):
    """Label 2 on two far-apart pixels (not connected), label 1 on the other two corners."""
    m = np.zeros((B, H, W), dtype=np.int32)
    m[:, 0, W - 1] = m[:, H - 1, 0] = 1
    m[:, 0, 0] = m[:, H - 1, W - 1] = 2
    return m


def _outside(B, H, W):
    """Labels 1 and 2 among negative ones, 2^31 - 1, -2^31 and labels above every M."""
    vals = np.array([-1, -7, -2 ** 31, 2 ** 31 - 1, 258, 300, 2 ** 30, 0, 1, 1, 2, 2], dtype=np.int64)
    return np.random.default_rng(9).choice(vals, (B, H, W)).astype(np.int32)


def _gap(B, H, W):
    """An empty image inside a batch: noise, nothing, one full component."""
    m = _noise3(B, H, W)
    m[1] = 0
    m[2:] = 1
    return m


FILLINGS = {"one": _one, "full": _full, "noise3": _noise3, "checker4": _checker4, "rings": _rings, "diagonal": _diagonal,
            "anti": _anti, "far": _far, "outside": _outside}
# (1,1,65) / (1,65,1): one more than a wave along a row / down a column; (3,17,129): more rows than a workgroup's items, three groups
# a row; (1,2,2100): a run longer than a group's carried span; the last two: the extent limit in each direction
FRAMES = ((1, 1, 1), (1, 1, 65), (1, 65, 1), (1, 2, 2), (3, 17, 129), (1, 2, 2100), (1, 8, 4096), (1, 4096, 8))


def lens(K=64):
    """One label whose right and left chains take the slopes K/2, (K-1)/2, .., -K/2 (a half-integer slope is an odd step over two
    rows): 2 (2 K + 2) strict vertices."""
    steps = [(1, m // 2) if m % 2 == 0 else (2, m) for m in range(K, -K - 1, -1)]         # (rows, dx), slopes strictly falling
    T, t = [0], 0
    for dy, dx in steps:
        if dy == 2:
            T.append(t + dx // 2)               # the lattice line between: floor of the chord, no vertex
        t += dx
        T.append(t)
    T = np.array(T, dtype=np.int64)
    half = int(T.max()) + 1
    H, W = len(T) - 1, 2 * half + 2
    m = np.zeros((1, H + 2, W), dtype=np.int32)
    for r in range(H):
        reach = int(min(T[r], T[r + 1]))        # a row's square must stay under the chain at both of its lattice lines
        m[0, r + 1, half - 1 - reach:half + 1 + reach + 1] = 1
    return m


def ties():
    """A filled square (both diagonals and all four edges tie), a 2 x 1 rectangle and a plus sign, one label each."""
    m = np.zeros((1, 16, 24), dtype=np.int32)
    m[0, 2:7, 1:6] = 1
    m[0, 9, 3:5] = 2
    m[0, 8:13, 14] = 3
    m[0, 10, 12:17] = 3
    return m


def wedges():
    """Three right triangles of 9 rows, one label each, the long side on the left chain, on the right chain, and below: the edge
    that decides the width runs upwards (negative ey), to the left (negative ex), or both.  Label 4 is a sliver whose one long
    straight side lies on the left chain and has no parallel edge on the right: its rectangle is flush with an edge that runs
    upwards."""
    m = np.zeros((1, 12, 70), dtype=np.int32)
    for r in range(9):
        m[0, 1 + r, 40 + 3 * r:40 + 3 * r + 2 + min(r, 8 - r)] = 4
    for r in range(9):
        m[0, 1 + r, 1 + r:10] = 1
        m[0, 1 + r, 14:15 + r] = 2
        m[0, 1 + r, 26 + 8 - r:26 + 9] = 3
    return m


def wide_positions():
    """The one 128-bit case: pixels (0, 0), (y, 0), (4095, 4095) and (4095 - y2, 4095) under one label in a 4096 x 4096 frame.  The
    pair (y, y2) is the first for which the two best width candidates C_i^2 / |e_i|^2 have cross-multiplied terms that both exceed
    2^64, differ, and compare the other way round when only their low 64 bits are kept -- so a 64-bit comparison picks the wrong
    edge."""
    for y in range(300, 420, 7):
        for y2 in range(300, 420, 5):
            pos = ((0, 0), (y, 0), (4095, 4095), (4095 - y2, 4095))
            V = vertices([p[0] for p in pos], [p[1] for p in pos])
            ev = edge_values(V)
            order = sorted(range(len(V)), key=lambda i: (Fraction(ev[i][2] ** 2, ev[i][0] ** 2 + ev[i][1] ** 2), i))
            i, j = order[0], order[1]
            l = ev[i][2] ** 2 * (ev[j][0] ** 2 + ev[j][1] ** 2)
            r = ev[j][2] ** 2 * (ev[i][0] ** 2 + ev[i][1] ** 2)
            if l >= 2 ** 64 and r >= 2 ** 64 and l < r and (l % 2 ** 64) > (r % 2 ** 64):
                return pos, (l, r)
    raise AssertionError("no pair of positions makes the 128-bit comparison matter")


def wide():
    pos, _ = wide_positions()
    m = np.zeros((1, 4096, 4096), dtype=np.int32)
    for y, x in pos:
        m[0, y, x] = 1
    return m


FIXED = {"lens": lens, "ties": ties, "wedges": wedges, "gap-3x17x129": lambda: _gap(3, 17, 129)}
CASES = [(f"{name}-{B}x{H}x{W}", name, (B, H, W)) for name in FILLINGS for (B, H, W) in FRAMES] + [(name, name, None) for name in FIXED]
CASE_IDS = [c[0] for c in CASES]
SMALL_IDS = [c[0] for c in CASES if c[2] is not None and c[2][1] * c[2][2] <= 17 * 129]      # where every pixel corner is checked


class Case:
    """labels int32 [B,H,W]; the reference table at the largest M (rows of a smaller M are its leading rows: a label's hull does
    not depend on the others), and per M the instance table."""

    def __init__(self, cid, name, shape):
        self.id = cid
        self.labels = np.ascontiguousarray(FIXED[name]() if shape is None else FILLINGS[name](*shape), dtype=np.int32)
        self._table, self._inst = None, {}

    def table(self, M):
        if self._table is None:
            self._table = table(self.labels, max(MS))
            self._table.setflags(write=False)
        return self._table[:, :M]

    def instances(self, M):
        if M not in self._inst:
            self._inst[M] = instance_table(self.labels, M)
        return self._inst[M]


@functools.lru_cache(maxsize=None)
def case(cid):
    if cid == "wide":
        c = Case.__new__(Case)
        c.id, c.labels, c._table, c._inst = cid, wide(), None, {}
        return c
    for c in CASES:
        if c[0] == cid:
            return Case(*c)
    raise KeyError(cid)
