"""The reference of the contour tests (tests/test_contours_host.py, tests/test_gpu_contours.py): a sequential tracer.  A dictionary
of directed edges keyed (Y, X, dir), the successor by the turn order (left, straight, right) for connectivity 8 and (right, straight,
left) for 4, rings collected from the sorted keys, Python integers throughout.  It shares nothing with the package's numpy path
(edge planes, pointer doubling, one lexsort) or with the kernels.  Also the case table both test files run and the checks that need
no reference: area, crack perimeter, Euler number, ring shape, even-odd rasterisation, scipy's component counts."""
import functools

import numpy as np
from scipy import ndimage

import hull_ref as HR

MS = (1, 3, 256, 257)
STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))          # (dy, dx) of E, S, W, N


def edges_of(lab, M):
    """{(Y, X, dir): label} of one image: the defect on the right of every edge."""
    H, W = lab.shape
    val = [[int(v) for v in row] for row in lab]
    out = {}
    for y in range(H):
        for x in range(W):
            k = val[y][x]
            if not 1 <= k <= M:
                continue
            if y == 0 or val[y - 1][x] != k:
                out[(y, x, 0)] = k
            if x == W - 1 or val[y][x + 1] != k:
                out[(y, x + 1, 1)] = k
            if y == H - 1 or val[y + 1][x] != k:
                out[(y + 1, x + 1, 2)] = k
            if x == 0 or val[y][x - 1] != k:
                out[(y + 1, x, 3)] = k
    return out


def trace(lab, M, connectivity):
    """The rings of one image in output order: dicts label, y, x, points [(y, x)], length, area2."""
    edges = edges_of(lab, M)
    turns = (3, 0, 1) if connectivity == 8 else (1, 0, 3)
    seen = set()
    rings = []
    for key in sorted(edges):
        if key in seen:
            continue
        k = edges[key]
        walk, cur = [], key
        while cur not in seen:
            seen.add(cur)
            walk.append(cur)
            Y, X, d = cur
            Y2, X2 = Y + STEP[d][0], X + STEP[d][1]
            nxt = [(Y2, X2, (d + t) % 4) for t in turns]
            nxt = [n for n in nxt if edges.get(n) == k]
            assert nxt, cur
            cur = nxt[0]
        assert cur == key                           # a cycle that closes where it began
        area2 = 0
        for Y, X, d in walk:
            Y2, X2 = Y + STEP[d][0], X + STEP[d][1]
            area2 += X * Y2 - X2 * Y
        points = [(Y, X) for i, (Y, X, d) in enumerate(walk) if walk[i - 1][2] != d]
        rings.append({"label": k, "y": key[0], "x": key[1], "points": points, "length": len(walk), "area2": area2})
    return rings


def tables(labels, M, connectivity, rings_per_image=None):
    """(points int32 [N,2], ring_offsets int32 [L+1], rings int64 [L,7], summary int64 [B,M,4]) of a batch.  rings_per_image: the
    trace at a larger M -- a label's rings do not depend on the other labels, so the rings of labels <= M are those of any M' >= M."""
    B = labels.shape[0]
    pts, rows, offs = [], [], [0]
    summary = np.zeros((B, M, 4), dtype=np.int64)
    for b in range(B):
        rings = rings_per_image[b] if rings_per_image is not None else trace(labels[b], M, connectivity)
        for r in rings:
            if r["label"] > M:
                continue
            rows.append([b, r["label"], r["y"], r["x"], len(r["points"]), r["length"], r["area2"]])
            pts += r["points"]
            offs.append(len(pts))
            summary[b, r["label"] - 1] += np.array([1, len(r["points"]), r["length"], r["area2"]], dtype=np.int64)
    return (np.array(pts, dtype=np.int32).reshape(-1, 2), np.array(offs, dtype=np.int32), np.array(rows, dtype=np.int64).reshape(-1, 7),
            summary)


# ------------------------------------------------------------------------------------------------ fillings: label maps [B,H,W] int32
def _checker(B, H, W):
    """Label 1 on every other pixel: every interior vertex is a saddle, the edge count is at its maximum."""
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat(((y + x) % 2 == 0).astype(np.int32)[None], B, axis=0)


def _nested(B, H, W):
    """Label 1 the frame's rim, label 2 all of its hole but a hole of its own, label 3 all of that: the hole ring of one label and
    the outer ring of the next start at the same vertex, twice."""
    m = np.ones((B, H, W), dtype=np.int32)
    if H > 2 and W > 2:
        m[:, 1:H - 1, 1:W - 1] = 2
    if H > 6 and W > 6:
        m[:, 3:H - 3, 3:W - 3] = 3
    return m


def _spiral(B, H, W):
    """A one-pixel-wide spiral of label 1 with one-pixel gaps, from the top left corner inwards: one ring of about H * W edges."""
    m = np.zeros((H, W), dtype=np.int32)
    y, x, d = 0, 0, 0
    m[0, 0] = 1
    free = lambda yy, xx: 0 <= yy < H and 0 <= xx < W and m[yy, xx] == 0
    stuck = 0
    while stuck < 2:
        dy, dx = STEP[d]
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        # go on while the next pixel is free and the one after it is not part of the spiral
        if free(y1, x1) and (not (0 <= y2 < H and 0 <= x2 < W) or m[y2, x2] == 0):
            y, x = y1, x1
            m[y, x] = 1
            stuck = 0
        else:
            d = (d + 1) % 4
            stuck += 1
    return np.repeat(m[None], B, axis=0)


def _comb(B, H, W):
    """The top row and every other column of label 1: a comb that fills the frame, one ring of about 2 * H * W edges."""
    m = np.zeros((B, H, W), dtype=np.int32)
    m[:, 0, :] = 1
    m[:, :, ::2] = 1
    return m


def _gap(B, H, W):
    m = HR._noise3(B, H, W)
    m[1] = 0
    m[2:] = 1
    return m


def _diag(which):
    m = np.zeros((3, 2, 2), dtype=np.int32)
    m[0] = [[1, 0], [0, 1]] if which == 0 else [[0, 1], [1, 0]]
    m[1] = [[1, 2], [2, 1]]
    m[2] = [[2, 1], [1, 300]]
    return m


FILLINGS = {"one": HR._one, "full": HR._full, "noise3": HR._noise3, "checker": _checker, "nested": _nested, "spiral": _spiral,
            "comb": _comb, "far": HR._far, "outside": HR._outside}
# (1,1,65) / (1,65,1): one more than a wave along a row / down a column; (3,17,129): several workgroups of vertices, a batch;
# (1,2,2100): more vertices a row than one workgroup scans; the last two: the extent limit in each direction, more edges than one
# workgroup of a scan holds
FRAMES = ((1, 1, 1), (1, 1, 65), (1, 65, 1), (1, 2, 2), (3, 17, 129), (1, 2, 2100), (1, 8, 4096), (1, 4096, 8))
FIXED = {"diag-main": lambda: _diag(0), "diag-anti": lambda: _diag(1), "gap-3x17x129": lambda: _gap(3, 17, 129),
         "empty-2x17x129": lambda: np.zeros((2, 17, 129), dtype=np.int32)}
CASES = [(f"{name}-{B}x{H}x{W}", name, (B, H, W)) for name in FILLINGS for (B, H, W) in FRAMES] + [(name, name, None) for name in FIXED]
CASE_IDS = [c[0] for c in CASES]


class Case:
    def __init__(self, cid, name, shape):
        self.id = cid
        self.labels = np.ascontiguousarray(FIXED[name]() if shape is None else FILLINGS[name](*shape), dtype=np.int32)
        self._rings, self._inst = {}, {}

    def tables(self, M, connectivity):
        """The reference outputs; traced once per connectivity at the largest M."""
        if connectivity not in self._rings:
            self._rings[connectivity] = [trace(self.labels[b], max(MS), connectivity) for b in range(self.labels.shape[0])]
        return tables(self.labels, M, connectivity, self._rings[connectivity])

    def instances(self, M):
        if M not in self._inst:
            self._inst[M] = HR.instance_table(self.labels, M)
        return self._inst[M]


@functools.lru_cache(maxsize=None)
def case(cid):
    for c in CASES:
        if c[0] == cid:
            return Case(*c)
    raise KeyError(cid)


# ------------------------------------------------------------------------------------------------ checks that need no reference
def rasterise(ring_points, H, W):
    """Even-odd fill of rings given as [n,2] arrays of (y, x) corner points: bool [H,W].  Every vertical side toggles the pixels to
    its right in the rows it spans."""
    acc = np.zeros((H, W + 1), dtype=np.int64)
    for p in ring_points:
        q = np.roll(p, -1, axis=0)
        for (y0, x0), (y1, x1) in zip(p.tolist(), q.tolist()):
            if x0 == x1:
                acc[min(y0, y1):max(y0, y1), x0] += 1
    return (np.cumsum(acc, axis=1)[:, :W] % 2).astype(bool)


def check_identities(labels, M, connectivity, points, offsets, rings, summary, inst_table, shape_props):
    """What holds for every correct output, whatever the reference says.  shape_props: shape_descriptors(...).props() at the same
    connectivity."""
    B, H, W = labels.shape
    assert offsets[0] == 0 and offsets[-1] == len(points) and len(offsets) == len(rings) + 1
    assert np.array_equal(np.diff(offsets), rings[:, 4])
    key = [tuple(r) for r in rings[:, [0, 2, 3]].tolist()]
    assert key == sorted(key)                                            # a raster order of the start vertices
    want = np.zeros((B, M, 4), dtype=np.int64)
    for r in rings:
        want[r[0], r[1] - 1] += [1, r[4], r[5], r[6]]
    assert np.array_equal(summary, want)
    assert np.array_equal(summary[..., 3], 2 * inst_table[..., 1])       # twice the pixel count
    on = inst_table[..., 1] > 0
    assert np.array_equal(summary[..., 2][on], shape_props["perimeter_crack"][on].astype(np.int64))
    assert not summary[~on].any()
    pos = np.zeros((B, M), dtype=np.int64)
    neg = np.zeros((B, M), dtype=np.int64)
    for i, r in enumerate(rings):
        p = points[offsets[i]:offsets[i + 1]]
        n = len(p)
        assert n >= 4 and n % 2 == 0 and r[6] != 0
        assert (p[0, 0], p[0, 1]) == (r[2], r[3]) == min(map(tuple, p.tolist()))       # starts at its smallest vertex
        assert sum(1 for q in p.tolist() if tuple(q) == (r[2], r[3])) == 1             # which it visits once
        step = np.roll(p, -1, axis=0) - p
        assert ((step != 0).sum(axis=1) == 1).all()                                    # one coordinate changes a side
        horizontal = step[:, 1] != 0
        assert (horizontal[::2] == horizontal[0]).all() and (horizontal[1::2] != horizontal[0]).all()
        assert (step[0, 1] > 0) if r[6] > 0 else (step[0, 0] > 0 and step[0, 1] == 0)  # heading E, or S for a hole
        assert np.abs(step).sum() == r[5]
        (pos if r[6] > 0 else neg)[r[0], r[1] - 1] += 1
    assert np.array_equal((pos - neg)[on], shape_props["euler"][on].astype(np.int64))  # components - holes
    four, eight = ndimage.generate_binary_structure(2, 1), np.ones((3, 3), dtype=bool)
    own, other = (eight, four) if connectivity == 8 else (four, eight)
    for b in range(B):
        present = np.nonzero(on[b])[0]
        for k in present[:6]:                                            # (a few labels an image: each costs an H x W plane)
            mine = [points[offsets[i]:offsets[i + 1]] for i in range(len(rings)) if rings[i, 0] == b and rings[i, 1] == k + 1]
            plane = labels[b] == k + 1
            assert np.array_equal(rasterise(mine, H, W), plane)
            assert ndimage.label(plane, structure=own)[1] == pos[b, k]
            assert ndimage.label(np.pad(~plane, 1, constant_values=True), structure=other)[1] - 1 == neg[b, k]
