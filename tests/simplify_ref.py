"""The reference of the simplification tests (tests/test_simplify_host.py, tests/test_gpu_simplify.py): the definition of
uaps_amd/simplify.py's docstring as an explicit-stack Ramer-Douglas-Peucker on Python integers (int64 arrays for the arg-max of a long
interval, whose bounds it asserts) over the rings of contours_ref.tables(...).  It shares nothing with the package's numpy path or
with the kernels.  Also the figures both test files run and check_properties, the checks that need no reference."""
import numpy as np

import contours_ref as CR

E16S = (0, 1, 8, 12, 16, 32, 128, 1024)


def deviation(P, A, B):
    """(num, den) of the point P against the segment A -> B; points are (y, x)."""
    dy, dx, qy, qx = B[0] - A[0], B[1] - A[1], P[0] - A[0], P[1] - A[1]
    L2, t = dy * dy + dx * dx, qy * dy + qx * dx
    if L2 == 0:
        return qy * qy + qx * qx, 1
    if t <= 0:
        return (qy * qy + qx * qx) * L2, L2
    if t >= L2:
        return ((P[0] - B[0]) ** 2 + (P[1] - B[1]) ** 2) * L2, L2
    return (dx * qy - dy * qx) ** 2, L2


def exceeds(num, den, e16):
    return 256 * num > e16 * e16 * den


def _worst(p, i, j, arr=None):
    """(num, index, den) of the interior index of (i, j) with the largest num, the lowest among the equal; None without one.
    arr: the ring as an int64 array, for the long intervals."""
    n, best = len(p), None
    if j - i > 48 and arr is not None:              # a long interval: the same four cases on int64 arrays (num <= 2^50 fits)
        a = arr[i + 1:j]
        A, B = p[i], p[j % n]
        dy, dx, qy, qx = B[0] - A[0], B[1] - A[1], a[:, 0] - A[0], a[:, 1] - A[1]
        L2, t, q2 = dy * dy + dx * dx, qy * dy + qx * dx, qy * qy + qx * qx
        if L2 == 0:
            num = q2
        else:
            end = ((a[:, 0] - B[0]) ** 2 + (a[:, 1] - B[1]) ** 2) * L2
            num = np.where(t <= 0, q2 * L2, np.where(t >= L2, end, (dx * qy - dy * qx) ** 2))
        k = int(np.argmax(num))                     # (the first of the equal)
        assert 0 <= int(num[k]) <= 2 ** 50 and L2 <= 2 ** 25
        return int(num[k]), i + 1 + k, max(L2, 1)
    for k in range(i + 1, j):
        num, den = deviation(p[k], p[i], p[j % n])
        assert 0 <= num <= 2 ** 50 and 1 <= den <= 2 ** 25
        if best is None or num > best[0]:
            best = (num, k, den)
    return best


def simplify_ring(p, e16):
    """(the kept indices of the ring p, a list of (y, x) tuples of Python integers, ascending; the depth of the recursion)."""
    n = len(p)
    assert n >= 4
    b = max(range(1, n), key=lambda i: ((p[i][0] - p[0][0]) ** 2 + (p[i][1] - p[0][1]) ** 2, -i))
    kept = {0, b}
    arr = np.array(p, dtype=np.int64).reshape(-1, 2)
    top = [(w, i, j) for (i, j) in ((0, b), (b, n)) for w in [_worst(p, i, j, arr)] if w is not None]
    stack = []
    if not any(exceeds(w[0], w[2], e16) for w, _, _ in top):            # never below a triangle
        w, i, j = max(top, key=lambda c: (c[0][0], -c[0][1]))
        assert w[0] > 0                                                 # a ring of non-zero area
        kept.add(w[1])
        stack += [(i, w[1], 2), (w[1], j, 2)]
    else:
        for w, i, j in top:
            if exceeds(w[0], w[2], e16):
                kept.add(w[1])
                stack += [(i, w[1], 2), (w[1], j, 2)]
    depth = 1
    while stack:
        i, j, d = stack.pop()
        w = _worst(p, i, j, arr)
        if w is None:
            continue
        depth = max(depth, d)
        if exceeds(w[0], w[2], e16):
            kept.add(w[1])
            stack += [(i, w[1], d + 1), (w[1], j, d + 1)]
    return sorted(kept), depth


_cache = {}


def kept_of(p, e16):
    key = (tuple(p), e16)
    if key not in _cache:
        _cache[key] = simplify_ring(list(p), e16)
    return _cache[key]


def shoelace(q):
    return sum(q[i][1] * q[(i + 1) % len(q)][0] - q[(i + 1) % len(q)][1] * q[i][0] for i in range(len(q)))


def simplified(tables, e16):
    """(points, ring_offsets, rings, summary, ring_stats) of the simplification of contours_ref.tables(...)'s four arrays."""
    points, offsets, rings, summary = tables
    pts = [tuple(int(v) for v in row) for row in points.tolist()]
    out, offs, stats = [], [0], []
    new_rings, new_summary = rings.copy(), summary.copy()
    for r in range(len(rings)):
        p = pts[offsets[r]:offsets[r + 1]]
        q = [p[i] for i in kept_of(p, e16)[0]]
        out += q
        offs.append(len(out))
        stats.append([len(p), shoelace(q)])
        new_rings[r, 4] = len(q)
        new_summary[rings[r, 0], rings[r, 1] - 1, 1] += len(q) - len(p)
    return (np.array(out, dtype=np.int32).reshape(-1, 2), np.array(offs, dtype=np.int32), new_rings, new_summary,
            np.array(stats, dtype=np.int64).reshape(-1, 2))


# ------------------------------------------------------------------------------------------------ checks that need no reference
def _brackets_hold(p, q, e16, need_tolerance):
    """Is q (kept points) a subsequence of the ring p that starts at p_0 -- and, with need_tolerance, one whose every dropped point
    does not exceed the tolerance against the segment between the kept points that bracket it?  A saddle vertex occurs twice in
    p, so a kept point can have two candidate indices; every choice is followed (at most two states a kept point)."""
    n = len(p)
    where = {}
    for i, v in enumerate(p):
        where.setdefault(v, []).append(i)

    def fits(i, j, B):
        return not need_tolerance or all(not exceeds(*deviation(p[k], p[i], B), e16) for k in range(i + 1, j))

    if not q or q[0] != p[0]:
        return False
    states = [0]
    for a in range(1, len(q)):
        states = [j for j in where.get(q[a], []) if any(i < j and fits(i, j, p[j]) for i in states)]
        if not states:
            return False
    return any(fits(i, n, p[0]) for i in states)


def check_properties(source, simplified_, e16, finer=None):
    """What holds for every correct output, whatever the reference says.  source: (points, ring_offsets, rings, summary);
    simplified_: (points, ring_offsets, rings, summary, ring_stats); finer: the simplified arrays at a tolerance <= e16 (P2)."""
    sp, so, sr, ss = source
    points, offsets, rings, summary, stats = simplified_
    L = len(sr)
    assert len(rings) == L and len(offsets) == L + 1 and stats.shape == (L, 2) and offsets[0] == 0 and offsets[-1] == len(points)
    assert np.array_equal(np.diff(offsets), rings[:, 4]) and np.array_equal(rings[:, [0, 1, 2, 3, 5, 6]], sr[:, [0, 1, 2, 3, 5, 6]])
    assert np.array_equal(stats[:, 0], sr[:, 4]) and (rings[:, 4] <= sr[:, 4]).all()
    want = ss.copy()
    for r in range(L):
        want[sr[r, 0], sr[r, 1] - 1, 1] += rings[r, 4] - sr[r, 4]
    assert np.array_equal(summary, want)
    if e16 == 0:                                                        # P1
        assert np.array_equal(points, sp) and np.array_equal(offsets, so) and np.array_equal(rings, sr) and np.array_equal(summary, ss)
    src, out = [tuple(v) for v in sp.tolist()], [tuple(v) for v in points.tolist()]
    fine = None if finer is None else [tuple(v) for v in finer[0].tolist()]
    for r in range(L):
        p, q = src[so[r]:so[r + 1]], out[offsets[r]:offsets[r + 1]]
        assert len(q) >= 3 and stats[r, 1] == shoelace(q), (r, q)
        # at least three points that are not collinear -- for a triangle that is a non-zero area.  A ring of more points can cross
        # itself (the definition does not promise otherwise) and a bow tie's shoelace sum can then cancel to exactly zero: ring 147
        # of noise3-3x17x129 at connectivity 8 becomes (4, 92), (8, 93), (7, 95), (9, 94) at e16 = 16, whose sum is 0
        w = next(v for v in q if v != q[0])
        assert any((w[1] - q[0][1]) * (v[0] - q[0][0]) - (w[0] - q[0][0]) * (v[1] - q[0][1]) != 0 for v in q), (r, q)
        assert len(q) > 3 or stats[r, 1] != 0, (r, q)
        assert _brackets_hold(p, q, e16, False), ("P4", r)
        assert _brackets_hold(p, q, e16, True), ("P3", r)
        if fine is not None:                                            # P2: the kept sets are nested
            f = fine[finer[1][r]:finer[1][r + 1]]
            assert _brackets_hold(f, q, 0, False), ("P2", r)


# ------------------------------------------------------------------------------------------------ figures: label maps [1,H,W] int32
def staircase(n=6):
    """A 45-degree staircase triangle: row y holds the pixels x <= y."""
    m = np.zeros((1, n, n), dtype=np.int32)
    for y in range(n):
        m[0, y, :y + 1] = 1
    return m


def rectangle(h=6, w=14):
    return np.ones((1, h, w), dtype=np.int32)


def plus(arm=3):
    m = np.zeros((1, 3 * arm, 3 * arm), dtype=np.int32)
    m[0, arm:2 * arm, :] = 1
    m[0, :, arm:2 * arm] = 1
    return m


def diamond(r=4):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (np.abs(y) + np.abs(x) <= r).astype(np.int32)[None]


def comb(teeth, bar_past_last=False, height=2):
    """A bar with `teeth` teeth below it: a ring of 4 * teeth points, or 4 * teeth + 2 with the bar one pixel past the last tooth."""
    m = np.zeros((1, height, 2 * teeth - 1 + (2 if bar_past_last else 0)), dtype=np.int32)
    m[0, 0, :] = 1
    m[0, :, 0:2 * teeth:2] = 1
    return m


def ramp_comb(teeth=64):
    """A bar with teeth of strictly increasing height: every round of the split rule peels one tooth."""
    m = np.zeros((1, teeth + 2, 2 * teeth - 1), dtype=np.int32)
    m[0, 0, :] = 1
    for t in range(teeth):
        m[0, :t + 3, 2 * t] = 1
    return m


def ring_tables(labels, M=1, connectivity=8):
    return CR.tables(np.ascontiguousarray(labels, dtype=np.int32), M, connectivity)


def drop_point(tables, ring=0, index=3):
    """The tables with one point of a ring taken out: a ring of an odd point count, which no trace gives."""
    points, offsets, rings, summary = (a.copy() for a in tables)
    at = offsets[ring] + index
    points = np.delete(points, at, axis=0)
    offsets[ring + 1:] -= 1
    rings[ring, 4] -= 1
    summary[rings[ring, 0], rings[ring, 1] - 1, 1] -= 1
    return points, offsets, rings, summary
