"""The reference of the rasterisation tests (tests/test_raster_host.py, tests/test_gpu_raster.py): a brute-force even-odd fill.  For
every label and every pixel centre it COUNTS the label's edges that cross the centre's row at or left of the centre, straight from
the definition -- an edge A -> B counts for pixel (r, c) iff min(2 ya, 2 yb) <= Yc < max(2 ya, 2 yb) and num <= (2 c + 1) s dy, with
Yc = (2 r + 1) s, s = 2^F and num = X0 dy + (Yc - Y0) dx from the doubled endpoint (Y0, X0) of smaller Y -- and a pixel belongs to
the label iff the count is odd; then the lowest label wins.  No column c0 is formed, nothing is toggled and nothing is scanned: it
shares neither the delta-and-scan of the kernels (csrc/raster.hip) nor the sorted crossing keys of the package's numpy path.

`count_python` is that count with Python integers, one pixel at a time; `plane_python_by_rows` is the same count, Python integers
too, with the edges that cross a row picked once a row.  `label_planes` evaluates the SAME inequality for a whole row of centres at
once on int64 arrays (every term stays below 2^40, so int64 is exact).  test_raster_host checks the Python-integer forms against
the array form on the polygon table and on the contour cases whose simplified rings overlap, traced and simplified; the rest of the
case table -- hundreds of fills of up to 6579 pixels times thousands of edges -- runs on the array form so that the suite stays
quick.  Also the polygon builders of the F = 4 table."""
import functools

import numpy as np

import contours_ref as R
import simplify_ref as S

E16S = (0, 12, 32, 1024)


def edges_of_ring(p):
    """[(Y0, X0, dy, dx)] of a ring given as [(y, x)]: doubled units, from the endpoint of smaller Y; horizontal edges left out."""
    out = []
    n = len(p)
    if n < 3:
        return out
    for i in range(n):
        (ya, xa), (yb, xb) = p[i], p[(i + 1) % n]
        ya, xa, yb, xb = 2 * int(ya), 2 * int(xa), 2 * int(yb), 2 * int(xb)
        if ya == yb:
            continue
        if ya < yb:
            out.append((ya, xa, yb - ya, xb - xa))
        else:
            out.append((yb, xb, ya - yb, xa - xb))
    return out


def count_python(edges, r, c, F):
    """How many of `edges` cross row r at or left of the centre of pixel (r, c): Python integers."""
    s = 1 << F
    Yc, Xc = (2 * r + 1) * s, (2 * c + 1) * s
    n = 0
    for Y0, X0, dy, dx in edges:
        if Y0 <= Yc < Y0 + dy and X0 * dy + (Yc - Y0) * dx <= Xc * dy:
            n += 1
    return n


def by_label(points, offsets, rings, B, M):
    """{(image, label): [edges]} of a ring set (the first two columns of `rings` are looked at)."""
    out = {}
    for i in range(len(rings)):
        b, k = int(rings[i, 0]), int(rings[i, 1])
        if 0 <= b < B and 1 <= k <= M:
            out.setdefault((b, k), []).extend(edges_of_ring(points[offsets[i]:offsets[i + 1]].tolist()))
    return out


def plane_python(edges, H, W, F):
    return np.array([[count_python(edges, r, c, F) & 1 for c in range(W)] for r in range(H)], dtype=bool).reshape(H, W)


def plane_python_by_rows(edges, H, W, F):
    """count_python's plane, still Python integers throughout, with the edges that cross a row picked once a row -- so that the
    contour cases (thousands of edges, few of them on any one row) can be counted this way too."""
    s = 1 << F
    plane = np.zeros((H, W), dtype=bool)
    for r in range(H):
        Yc = (2 * r + 1) * s
        live = [(X0 * dy + (Yc - Y0) * dx, dy) for Y0, X0, dy, dx in edges if Y0 <= Yc < Y0 + dy]
        if live:
            plane[r] = [sum(1 for num, dy in live if num <= (2 * c + 1) * s * dy) & 1 for c in range(W)]
    return plane


def plane_arrays(edges, H, W, F):
    """The same plane, a row of centres at a time on int64 arrays."""
    plane = np.zeros((H, W), dtype=bool)
    if not edges:
        return plane
    s = 1 << F
    E = np.array(edges, dtype=np.int64)
    Y0, X0, dy, dx = E[:, 0], E[:, 1], E[:, 2], E[:, 3]
    assert int(np.abs(E).max()) < 1 << 19                               # every product below stays under 2^40
    Xc = (2 * np.arange(W, dtype=np.int64) + 1) * s
    lo = max(0, int((Y0.min() - s) // (2 * s)))
    hi = min(H - 1, int(((Y0 + dy).max() - s) // (2 * s)))
    for r in range(lo, hi + 1):
        Yc = (2 * r + 1) * s
        sel = (Y0 <= Yc) & (Yc < Y0 + dy)
        if not sel.any():
            continue
        num, d = X0[sel] * dy[sel] + (Yc - Y0[sel]) * dx[sel], dy[sel]
        count = np.zeros(W, dtype=np.int64)
        for a in range(0, len(num), 512):                               # (512 edges a trip: the comparison's table stays small)
            count += (num[a:a + 512, None] <= Xc[None, :] * d[a:a + 512, None]).sum(axis=0)
        plane[r] = (count & 1) == 1
    return plane


def label_planes(points, offsets, rings, B, H, W, M, F, python=False):
    """{(image, label): bool [H,W]} of every label with an edge."""
    fill = plane_python if python else plane_arrays
    return {key: fill(edges, H, W, F) for key, edges in by_label(points, offsets, rings, B, M).items()}


def compose(planes, B, H, W, M, background=0, reference=None, classes=None):
    """(labels int64 [B,H,W], mask or None, stats int64 [B,M,2], overlap int64 [B], cover int64 [B,H,W]) by the lowest-label rule;
    planes of labels above M are left out (a label's fill does not depend on the other labels)."""
    labels = np.full((B, H, W), background, dtype=np.int64)
    owned = np.zeros((B, H, W), dtype=bool)
    cover = np.zeros((B, H, W), dtype=np.int64)
    stats = np.zeros((B, M, 2), dtype=np.int64)
    for (b, k) in sorted(planes, reverse=True):                         # descending: the lowest label is written last
        if k > M:
            continue
        p = planes[(b, k)]
        labels[b][p] = k
        owned[b] |= p
        cover[b] += p
        stats[b, k - 1, 0] = int(p.sum())
        if reference is not None:
            stats[b, k - 1, 1] = int((p & (reference[b] == k)).sum())
    mask = None
    if classes is not None:
        mask = np.zeros((B, H, W), dtype=np.int64)
        for b in range(B):
            mask[b][owned[b]] = classes[b][labels[b][owned[b]] - 1]
    return labels, mask, stats, (cover >= 2).reshape(B, -1).sum(axis=1).astype(np.int64), cover


def iou_fractions(stats, ref_area):
    """[[Fraction or None]] of inter / (reference area + area - inter)."""
    from fractions import Fraction
    B, M = stats.shape[:2]
    out = []
    for b in range(B):
        row = []
        for k in range(M):
            union = int(ref_area[b, k]) + int(stats[b, k, 0]) - int(stats[b, k, 1])
            row.append(Fraction(int(stats[b, k, 1]), union) if union > 0 else None)
        out.append(row)
    return out


# ------------------------------------------------------------------------------------------------ the contour case table
@functools.lru_cache(maxsize=None)
def case_tables(cid, conn, e16):
    """(points, ring_offsets, rings) of a contour case at the largest M: traced (e16 None) or simplified."""
    t = R.case(cid).tables(max(R.MS), conn)
    return t[:3] if e16 is None else S.simplified(t, e16)[:3]


@functools.lru_cache(maxsize=None)
def case_planes(cid, conn, e16):
    """The per-label planes of a contour case, computed once at the largest M and shared by every M and every test."""
    B, H, W = R.case(cid).labels.shape
    return label_planes(*case_tables(cid, conn, e16), B, H, W, max(R.MS), 0)


def case_reference(cid, conn, e16, M, background=0, classes=None):
    labels = R.case(cid).labels
    B, H, W = labels.shape
    return compose(case_planes(cid, conn, e16), B, H, W, M, background, labels, classes)


def rings_upto(tables, M):
    """The rings of labels <= M of (points, ring_offsets, rings): what contours / simplify_contours return at that M."""
    points, offsets, rings = tables
    keep = [i for i in range(len(rings)) if rings[i, 1] <= M]
    pts = [points[offsets[i]:offsets[i + 1]] for i in keep]
    out_p = np.concatenate(pts).astype(np.int32) if pts else np.zeros((0, 2), dtype=np.int32)
    return out_p, np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32), rings[keep].reshape(-1, rings.shape[1])


# ------------------------------------------------------------------------------------------------ the F = 4 polygon table
F4 = 4
PX = 1 << F4


def _convex(q):
    n = len(q)
    sign = 0
    for i in range(n):
        (y0, x0), (y1, x1), (y2, x2) = q[i], q[(i + 1) % n], q[(i + 2) % n]
        cr = (x1 - x0) * (y2 - y1) - (y1 - y0) * (x2 - x1)
        if cr == 0 or (sign and (cr > 0) != (sign > 0)):
            return False
        sign = cr
    return True


def random_quads(seed, count, H, W):
    """`count` strictly convex quads in sixteenths of a pixel inside and around an H x W frame, 60 % of their coordinates snapped
    onto pixel centres (16 r + 8): vertices lie on centre rows and edges pass through centres."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        cy, cx = rng.uniform(1, H - 1), rng.uniform(1, W - 1)
        rad = rng.uniform(1.5, max(H, W) * 0.6)
        ang = np.sort(rng.uniform(0, 2 * np.pi, 4))
        q = []
        for a in ang:
            y = int(round(max(0.0, cy + rad * np.sin(a)) * PX))
            x = int(round(max(0.0, cx + rad * np.cos(a)) * PX))
            if rng.random() < 0.6:
                y = (y // PX) * PX + PX // 2
            if rng.random() < 0.6:
                x = (x // PX) * PX + PX // 2
            q.append((y, x))
        if _convex(q):
            out.append(q)
    return out


def tables_of(rows):
    """(points int32 [N,2], ring_offsets int32 [L+1], rings int64 [L,2]) of rows (image, label, [(y, x)])."""
    pts = [np.array(r[2], dtype=np.int32).reshape(-1, 2) for r in rows]
    points = np.concatenate(pts) if pts else np.zeros((0, 2), dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
    return points, offsets, np.array([[r[0], r[1]] for r in rows], dtype=np.int64).reshape(-1, 2)


def quad_tables(seed, count, H, W, reverse=False, diagonal=0):
    """Two ring sets over `count` images, a quad an image: the two triangles of one diagonal as labels 1 and 2, and the quad as
    label 1.  reverse: every ring in the other orientation; diagonal: which of the two diagonals splits the quad."""
    tris, quads = [], []
    for b, q in enumerate(random_quads(seed, count, H, W)):
        q = q[diagonal:] + q[:diagonal]
        t1, t2, whole = [q[0], q[1], q[2]], [q[0], q[2], q[3]], list(q)
        if reverse:
            t1, t2, whole = t1[::-1], t2[::-1], whole[::-1]
        tris += [(b, 1, t1), (b, 2, t2)]
        quads.append((b, 1, whole))
    return tables_of(tris), tables_of(quads)


def _px(*yx):
    return [(int(round(y * PX)), int(round(x * PX))) for y, x in yx]


def polygon_cases():
    """{name: (tables, B, M, H, W)} at F = 4: the figures the fill rule can get wrong."""
    cases = {}
    # polygons that reach outside the frame: over the right and bottom sides, one wholly right of it (every crossing at c0 = W), one
    # over the corner at the origin, one as large as the coordinate range
    big = 4096 * PX
    cases["outside"] = (tables_of([(0, 1, _px((2.25, 3.5), (4.5, 40.0), (30.0, 20.0), (6.0, 1.0))),
                                   (0, 2, _px((1.0, 14.5), (1.0, 30.0), (8.0, 30.0), (8.0, 14.5))),
                                   (0, 3, _px((0.0, 0.0), (0.0, 2.5), (2.5, 0.0))),
                                   (1, 1, [(0, 0), (0, big), (big, big), (big, 0)]),
                                   (1, 2, _px((3.5, 3.5), (3.5, 9.5), (7.5, 9.5), (7.5, 3.5)))]), 2, 3, 9, 12)
    # rings of two points and of one contribute nothing; a triangle beside them does
    cases["two-points"] = (tables_of([(0, 1, _px((1.0, 1.0), (6.0, 7.0))), (0, 2, _px((2.0, 2.0))),
                                      (0, 3, _px((1.5, 1.5), (1.5, 6.5), (6.5, 1.5))), (0, 1, _px((0.5, 0.5), (3.5, 0.5)))]), 1, 3, 8, 8)
    # vertices on centre rows and columns, edges through centres: a diamond with its four vertices on pixel centres, a square whose
    # sides run along centre rows and centre columns, a slanted edge through a row of centres
    cases["centres"] = (tables_of([(0, 1, _px((0.5, 4.5), (4.5, 8.5), (8.5, 4.5), (4.5, 0.5))),
                                   (1, 1, _px((1.5, 1.5), (1.5, 6.5), (6.5, 6.5), (6.5, 1.5))),
                                   (2, 1, _px((0.5, 0.5), (8.5, 8.5), (8.5, 0.5))),
                                   (2, 2, _px((0.5, 0.5), (0.5, 8.5), (8.5, 8.5)))]), 3, 2, 10, 10)
    # the same figures in the other orientation
    fwd = cases["centres"][0]
    cases["centres-reversed"] = (tables_of([(int(fwd[2][i, 0]), int(fwd[2][i, 1]), fwd[0][fwd[1][i]:fwd[1][i + 1]][::-1].tolist())
                                            for i in range(len(fwd[2]))]), 3, 2, 10, 10)
    # even-odd: a pentagram's centre is out, a bow tie, a hole ring of the same label, another label inside the hole, two labels that
    # overlap (the lowest wins), one label drawn twice (it cancels itself)
    star = _px(*[(8 + 7 * np.sin(2 * np.pi * (2 * i) / 5), 8 + 7 * np.cos(2 * np.pi * (2 * i) / 5)) for i in range(5)])
    cases["even-odd"] = (tables_of([(0, 1, star),
                                    (1, 1, _px((1.0, 1.0), (12.0, 13.0), (12.0, 1.0), (1.0, 13.0))),
                                    (2, 2, _px((1.0, 1.0), (1.0, 14.0), (14.0, 14.0), (14.0, 1.0))),
                                    (2, 2, _px((4.0, 4.0), (11.0, 4.0), (11.0, 11.0), (4.0, 11.0))),
                                    (2, 5, _px((5.25, 5.25), (5.25, 9.75), (9.75, 9.75))),
                                    (3, 3, _px((2.0, 2.0), (2.0, 10.0), (10.0, 10.0), (10.0, 2.0))),
                                    (3, 1, _px((6.0, 6.0), (6.0, 15.0), (15.0, 15.0), (15.0, 6.0))),
                                    (3, 4, _px((1.0, 12.0), (1.0, 15.0), (4.0, 15.0), (4.0, 12.0))),
                                    (3, 4, _px((1.0, 12.0), (1.0, 15.0), (4.0, 15.0), (4.0, 12.0)))]), 4, 5, 16, 16)
    # pixels of three and four owners, the lowest label neither the first nor the last of them
    cases["stack"] = (tables_of([(0, 3, _px((0.0, 0.0), (0.0, 12.0), (12.0, 12.0), (12.0, 0.0))),
                                 (0, 1, _px((3.0, 3.0), (3.0, 9.0), (9.0, 9.0), (9.0, 3.0))),
                                 (0, 4, _px((1.0, 1.0), (1.0, 7.0), (7.0, 7.0), (7.0, 1.0))),
                                 (0, 2, _px((5.0, 0.0), (5.0, 12.0), (11.0, 6.0)))]), 1, 4, 12, 12)
    # labels and images outside the table are left out; a wide frame: boxes that start at columns 63, 64 and 65 and cross words
    cases["wide"] = (tables_of([(0, 1, _px((0.0, 63.0), (0.0, 130.0), (3.0, 130.0), (3.0, 63.0))),
                                (0, 2, _px((1.0, 64.0), (1.0, 66.0), (3.0, 66.0), (3.0, 64.0))),
                                (0, 3, _px((0.25, 65.0), (2.75, 200.0), (2.75, 65.0))),
                                (0, 9, _px((0.0, 0.0), (0.0, 5.0), (3.0, 5.0))), (7, 1, _px((0.0, 0.0), (0.0, 5.0), (3.0, 5.0))),
                                (0, 0, _px((0.0, 0.0), (0.0, 5.0), (3.0, 5.0)))]), 1, 3, 3, 200)
    return cases
