"""Convex hulls without a GPU: the package's CPU restatement (uaps_amd/hull.py: row extents and two lattice-line chains) against the
brute-force reference (tests/hull_ref.py: all pixel corners, sorted monotone chain, Fraction) bit for bit on the case table; the
inequalities that tie every row to the instance table's area and box; scipy's qhull for the area; props() and rect_corners() against
the same formulas in Fraction and math; records(), the argument checks, the C ABI's refusals (they return before any launch) and the
hull= keyword of inference.predict_instances around a stub network."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull

import hull_ref as R
from conftest import ROOT
from test_bn_ref import norm_act_kernel_symbols

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3


def _inst(case, M):
    from uaps_amd.instances import InstanceResult
    count, table = case.instances(M)
    return InstanceResult(torch.from_numpy(case.labels), torch.from_numpy(count), torch.from_numpy(table), 0)


def test_error_codes_are_those_of_the_header():
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"(UAPS_E[A-Z]+)\s*=\s*(-?\d+)", text)}
    codes.update({k: int(v) for k, v in re.findall(r"#define (UAPS_E[A-Z]+) \(?(-?\d+)\)?", text)})
    assert (codes["UAPS_EINVAL"], codes["UAPS_ERANGE"], codes["UAPS_EWORKSPACE"]) == (EINVAL, ERANGE, EWORKSPACE)


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_cpu_path_equals_the_reference_and_the_bounds_hold(cid):
    from uaps_amd import hull_descriptors
    case = R.case(cid)
    for M in R.MS:
        res = hull_descriptors(_inst(case, M))
        assert res.table.dtype == torch.int64 and tuple(res.table.shape) == (case.labels.shape[0], M, 17) and res.also is None
        got, ref = res.table.numpy(), case.table(M)
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (cid, M, bad[:4], got[tuple(bad[0][:2])], ref[tuple(bad[0][:2])])
    _bounds(case, R.MS[-1], case.table(R.MS[-1]))


def _bounds(case, M, t):
    _, itab = case.instances(M)
    area, bh, bw = itab[..., 1], itab[..., 4] - itab[..., 2], itab[..., 5] - itab[..., 3]
    on = area > 0
    assert ((t == 0).all(axis=-1) == ~on).all()                         # a row is zero exactly where no pixel carries the label
    if not on.any():
        return
    t, area, bh, bw = t[on], area[on], bh[on], bw[on]
    nv, area2, fsq, wey, wex, wc = t[:, 0], t[:, 1], t[:, 2], t[:, 7], t[:, 8], t[:, 9]
    rey, rex, dmin, dmax, rc = (t[:, c] for c in (12, 13, 14, 15, 16))
    assert (nv >= 4).all() and (area2 >= 2 * area).all()
    rect = area == bh * bw
    assert (area2[rect] == 2 * area[rect]).all() and (nv[rect] == 4).all()
    assert (np.maximum(bh, bw) ** 2 <= fsq).all() and (fsq <= bh * bh + bw * bw).all()
    assert ((t[:, 3] < t[:, 5]) | ((t[:, 3] == t[:, 5]) & (t[:, 4] < t[:, 6]))).all()
    assert ((t[:, 5] - t[:, 3]) ** 2 + (t[:, 6] - t[:, 4]) ** 2 == fsq).all()
    E, F = wex * wex + wey * wey, rex * rex + rey * rey
    for i in range(len(t)):                                             # (the products pass 2^63: Python integers)
        assert int(wc[i]) ** 2 <= min(int(bh[i]), int(bw[i])) ** 2 * int(E[i])
        mid = 2 * int(dmax[i] - dmin[i]) * int(rc[i])
        assert int(area2[i]) * int(F[i]) <= mid <= 2 * int(bh[i]) * int(bw[i]) * int(F[i])
        assert dmin[i] <= 0 and dmax[i] >= F[i] and rc[i] > 0


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_hull_area_equals_qhull(cid):
    case = R.case(cid)
    M = R.MS[-1]
    t = case.table(M)
    checked = 0
    for b in range(case.labels.shape[0]):
        for k in np.nonzero(t[b, :, 0])[0][:40]:
            y, x = np.nonzero(case.labels[b] == k + 1)
            corners = np.unique(np.concatenate([np.stack([x + dx, y + dy], axis=1) for dy in (0, 1) for dx in (0, 1)]), axis=0)
            assert t[b, k, 1] > 0
            assert t[b, k, 1] / 2 == pytest.approx(ConvexHull(corners.astype(np.float64)).volume, rel=1e-9), (cid, b, k)
            checked += 1
    assert checked > 0 or not t.any()


@pytest.mark.parametrize("cid", R.SMALL_IDS + ["ties"])
def test_every_pixel_corner_lies_inside_every_edge(cid):
    case = R.case(cid)
    for b in range(case.labels.shape[0]):
        for k in range(1, 4):
            y, x = np.nonzero(case.labels[b] == k)
            if len(y) == 0:
                continue
            V = R.vertices(y, x)
            assert len(V) == case.table(3)[b, k - 1, 0] and V[0][1] == V[1][1] and V[1][0] - V[0][0] >= 1       # a horizontal top edge
            assert (V[0][1], V[0][0]) == min((p[1], p[0]) for p in V)
            px = np.concatenate([x, x + 1, x, x + 1]).astype(np.int64)
            py = np.concatenate([y, y, y + 1, y + 1]).astype(np.int64)
            for i, (vx, vy) in enumerate(V):
                ex, ey = V[(i + 1) % len(V)][0] - vx, V[(i + 1) % len(V)][1] - vy
                c = ex * (py - vy) - ey * (px - vx)
                assert c.min() == 0 and (c == 0).sum() >= 2, (cid, b, k, i)


def test_the_case_table_is_informative():
    ids = R.CASE_IDS
    assert len(ids) == len(set(ids))
    lens = R.case("lens")
    assert lens.table(1)[0, 0, 0] > R.THREADS > 64 and lens.labels.shape[1] < 200 and lens.labels.shape[2] <= 4096
    assert R.case("full-1x2x2100").labels.shape[2] > 2 * 16 * 64         # crosses the carried span twice
    assert R.case("checker4-1x8x4096").labels.max() > 4 * R.MS[-1]       # far more labels than rows
    assert len(np.unique(R.case("checker4-3x17x129").labels[0, 0, :64])) >= 16          # many labels in one group of lanes
    far = R.case("far-3x17x129")
    assert far.table(3)[0, 1].tolist()[:7] == [6, 2 * (17 + 129 - 1), 17 ** 2 + 129 ** 2, 0, 0, 17, 129]
    rings = R.case("rings-3x17x129").table(3)[0]
    assert rings[0, 1] == 2 * 17 * 129 and rings[1, 1] == 2 * 13 * 125 and 0 < rings[2, 1] < rings[1, 1]
    out = R.case("outside-3x17x129")
    assert out.labels.min() == -2 ** 31 and out.labels.max() == 2 ** 31 - 1 and (out.table(257)[:, 2:] == 0).all()
    gap = R.case("gap-3x17x129")
    assert not gap.labels[1].any() and not gap.table(3)[1].any() and gap.table(3)[0].any() and gap.table(3)[2, 0, 1] == 2 * 17 * 129
    seen = np.zeros(17, dtype=bool)
    neg = np.zeros(17, dtype=bool)
    for cid in ids:
        t = R.case(cid).table(R.MS[-1])
        seen |= (t != 0).any(axis=(0, 1))
        neg |= (t < 0).any(axis=(0, 1))
    assert seen.all()                                                   # every column is non-zero somewhere
    assert neg[[7, 8, 12, 13, 14]].all() and not neg[[0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 15, 16]].any()       # the signed ones are negative somewhere


def test_tie_figures_are_decided_by_the_tie_rules():
    t = R.case("ties").table(3)[0]
    # a 5 x 5 square at (2, 1): both diagonals tie -> the pair from the smallest vertex; all four edges tie -> edge 0, the top one
    assert t[0].tolist() == [4, 50, 50, 2, 1, 7, 6, 0, 5, 25, 2, 1, 0, 5, 0, 25, 25]
    # a 2 x 1 rectangle: width along edge 0 (height 1); both diagonals tie
    assert t[1].tolist() == [4, 4, 5, 9, 3, 10, 5, 0, 2, 2, 9, 3, 0, 2, 0, 4, 2]
    assert t[2, 0] == 8 and t[2, 1] == 34
    one = R.case("one-1x1x1").table(1)[0, 0]
    assert one.tolist() == [4, 2, 2, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1]           # 4 vertices, area 1, sqrt(2), width 1


def test_the_wide_case_needs_128_bits():
    pos, (l, r) = R.wide_positions()
    assert l >= 2 ** 64 and r >= 2 ** 64 and l != r and (l < r) != (l % 2 ** 64 < r % 2 ** 64)
    from uaps_amd import hull_descriptors
    case = R.case("wide")
    assert case.labels.shape == (1, 4096, 4096) and int((case.labels != 0).sum()) in (3, 4)
    res = hull_descriptors(_inst(case, 1))
    assert np.array_equal(res.table.numpy(), case.table(1))


def _ulps(got, want):
    return got == want or abs(got - want) <= 4 * math.ulp(want)


def _angle(dx, dy):
    if dx < 0 or (dx == 0 and dy < 0):
        dx, dy = -dx, -dy
    return math.atan2(dy, dx)


@pytest.mark.parametrize("cid", ("ties", "noise3-3x17x129", "rings-3x17x129", "lens", "diagonal-1x65x1", "anti-3x17x129", "far-1x2x2100"))
def test_props_and_corners_against_fractions(cid):
    from uaps_amd import hull_descriptors
    from uaps_amd.hull import PROPS
    case = R.case(cid)
    M = 3
    res = hull_descriptors(_inst(case, M))
    p, corners = res.props(), res.rect_corners()
    assert tuple(p) == PROPS and corners.shape == (case.labels.shape[0], M, 4, 2) and corners.dtype == np.float64
    t, itab = case.table(M), case.instances(M)[1]
    for b in range(t.shape[0]):
        for k in range(M):
            if itab[b, k, 1] == 0:
                assert all(np.isnan(v[b, k]) for v in p.values()) and np.isnan(corners[b, k]).all()
                continue
            nv, area2, fsq, fy0, fx0, fy1, fx1, wey, wex, wc, ry, rx, rey, rex, dmin, dmax, rc = (int(v) for v in t[b, k])
            A, E, F, D = int(itab[b, k, 1]), wex ** 2 + wey ** 2, rex ** 2 + rey ** 2, dmax - dmin
            along, across = math.sqrt(Fraction(D * D, F)), math.sqrt(Fraction(rc * rc, F))
            want = {"hull_vertices": float(nv), "hull_area": float(Fraction(area2, 2)), "solidity": float(Fraction(2 * A, area2)),
                    "feret_max": math.sqrt(fsq), "feret_max_angle": _angle(fx1 - fx0, fy1 - fy0),
                    "feret_min": math.sqrt(Fraction(wc * wc, E)), "feret_min_angle": _angle(-wey, wex),
                    "feret_aspect": math.sqrt(Fraction(wc * wc, E * fsq)),
                    "rect_length": max(along, across), "rect_width": min(along, across), "rect_area": float(Fraction(D * rc, F)),
                    "rect_angle": _angle(rex, rey) if D >= rc else _angle(-rey, rex),
                    "rect_cy": float(ry + Fraction((dmin + dmax) * rey + rc * rex, 2 * F)),
                    "rect_cx": float(rx + Fraction((dmin + dmax) * rex - rc * rey, 2 * F)),
                    "rectangularity": float(Fraction(A * F, D * rc))}
            for name, w in want.items():
                assert _ulps(float(p[name][b, k]), w), (cid, b, k, name, p[name][b, k], w)
            assert p["solidity"][b, k] <= 1.0 and p["feret_aspect"][b, k] <= 1.0 and p["rectangularity"][b, k] <= 1.0
            assert -math.pi / 2 < p["rect_angle"][b, k] <= math.pi / 2 and p["rect_length"][b, k] >= p["rect_width"][b, k]
            for j, (d, c) in enumerate(((dmin, 0), (dmax, 0), (dmax, rc), (dmin, rc))):
                wy = float(ry + Fraction(d * rey + c * rex, F))
                wx = float(rx + Fraction(d * rex - c * rey, F))
                assert _ulps(corners[b, k, j, 0], wy) and _ulps(corners[b, k, j, 1], wx), (cid, b, k, j)
            cy, cx = corners[b, k, :, 0].mean(), corners[b, k, :, 1].mean()
            assert cy == pytest.approx(p["rect_cy"][b, k], rel=1e-12, abs=1e-9) and cx == pytest.approx(p["rect_cx"][b, k], rel=1e-12, abs=1e-9)
            # the rectangle holds every hull vertex: its corners, taken in order, have every vertex on their inner side
            y, x = np.nonzero(case.labels[b] == k + 1)
            for j in range(4):
                (ay, ax), (by, bx) = corners[b, k, j], corners[b, k, (j + 1) % 4]
                side = (bx - ax) * (np.concatenate([y, y + 1]) - ay) - (by - ay) * (np.concatenate([x, x + 1]) - ax)
                assert side.min() >= -1e-6 * (1 + abs(side).max())


def test_props_of_known_figures():
    from uaps_amd import hull_descriptors
    res = hull_descriptors(_inst(R.case("ties"), 3))
    p = {k: v[0] for k, v in res.props().items()}
    assert p["hull_area"].tolist() == [25.0, 2.0, 17.0] and p["solidity"].tolist()[:2] == [1.0, 1.0] and p["solidity"][2] == 9 / 17
    assert p["feret_max"].tolist() == [math.sqrt(50), math.sqrt(5), math.sqrt(26)] and p["feret_min"].tolist()[:2] == [5.0, 1.0]
    assert p["rect_length"].tolist()[:2] == [5.0, 2.0] and p["rect_width"].tolist()[:2] == [5.0, 1.0] and p["rect_angle"].tolist()[:2] == [0.0, 0.0]
    assert p["rect_cy"].tolist()[:2] == [4.5, 9.5] and p["rect_cx"].tolist()[:2] == [3.5, 4.0] and p["rectangularity"].tolist()[:2] == [1.0, 1.0]
    assert p["feret_max_angle"][0] == pytest.approx(math.pi / 4) and p["feret_min_angle"][0] == pytest.approx(math.pi / 2)
    assert res.rect_corners()[0, 1].tolist() == [[9.0, 3.0], [9.0, 5.0], [10.0, 5.0], [10.0, 3.0]]
    tall = hull_descriptors(_inst(R.case("full-1x65x1"), 1))
    q = {k: float(v[0, 0]) for k, v in tall.props().items()}
    assert (q["rect_length"], q["rect_width"], q["feret_min"], q["hull_vertices"]) == (65.0, 1.0, 1.0, 4.0)
    assert q["rect_angle"] == pytest.approx(math.pi / 2) and q["feret_max"] == math.sqrt(65 ** 2 + 1)
    dot = hull_descriptors(_inst(R.case("one-1x1x1"), 1)).props()
    assert dot["hull_area"][0, 0] == 1.0 and dot["feret_max"][0, 0] == math.sqrt(2.0) and dot["feret_min"][0, 0] == 1.0


class Shaped:
    """Stands for a ShapeResult / SkeletonStats in `also`: records() of its own."""

    def __init__(self, inst):
        self.inst = inst

    def records(self):
        recs = self.inst.records()
        for rows in recs:
            for r in rows:
                r["extra"] = 7.0
        return recs


def test_records_merge_with_also():
    from uaps_amd import hull_descriptors
    from uaps_amd.hull import PROPS
    res = hull_descriptors(_inst(R.case("rings-3x17x129"), 3))
    recs, p = res.records(), res.props()
    assert len(recs) == 3 and [r["label"] for r in recs[0]] == [1, 2, 3]
    assert set(PROPS) <= set(recs[0][0]) and "extra" not in recs[0][0] and recs[0][0]["area"] == int(res.instances.table[0, 0, 1])
    assert all(recs[b][k][n] == float(p[n][b, k]) for b in range(3) for k in range(3) for n in PROPS)
    merged = res._replace(also=Shaped(res.instances)).records()
    assert merged[1][2]["extra"] == 7.0 and merged[1][2]["solidity"] == recs[1][2]["solidity"] and set(recs[0][0]) < set(merged[0][0])


def test_argument_checks():
    from uaps_amd import hull_descriptors, label_instances
    from uaps_amd.instances import InstanceResult
    inst = label_instances(torch.ones(1, 4, 4, dtype=torch.int64))
    assert hull_descriptors(inst).table.shape == (1, 256, 17)
    for bad in (inst.labels, (inst.labels, inst.count, inst.table), None):
        with pytest.raises(TypeError, match="hull_descriptors: an instances.InstanceResult expected"):
            hull_descriptors(bad)
    for labels in (inst.labels.long(), inst.labels[0], inst.labels.float()):
        with pytest.raises(TypeError, match=r"hull_descriptors: int32 \[B,H,W\] labels expected"):
            hull_descriptors(InstanceResult(labels, inst.count, inst.table))
    with pytest.raises(TypeError, match="the instance table is int64"):
        hull_descriptors(InstanceResult(inst.labels, inst.count, inst.table[..., :8]))
    with pytest.raises(ValueError, match="hull_descriptors: H and W up to 4096"):
        hull_descriptors(InstanceResult(torch.zeros(1, 1, 4097, dtype=torch.int32), inst.count, inst.table))
    with pytest.raises(ValueError, match="hull_descriptors: empty labels"):
        hull_descriptors(InstanceResult(torch.zeros(1, 0, 4, dtype=torch.int32), inst.count, inst.table))
    big = torch.zeros(1, 1, 1, dtype=torch.int32).expand(64, 2048, 2048)
    with pytest.raises(ValueError, match="2 GiB"):
        hull_descriptors(InstanceResult(big, inst.count.expand(64), inst.table.expand(64, 256, 9)))


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib, hull
    import uaps_amd
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("uaps_hull_descriptors", "uaps_hull_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_hull_call \{(.*?)\} uaps_hull_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.HullCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_HULL_[A-Z_]+) (\d+)", text))
    assert int(defines["UAPS_HULL_COLUMNS"]) == _lib.HULL_COLUMNS == len(hull.HULL_COLUMNS) == 17 and hull.HULL_COLUMNS == R.COLUMNS
    assert int(defines["UAPS_HULL_MAX_EXTENT"]) == _lib.HULL_MAX_EXTENT == hull.MAX_EXTENT == 4096
    assert C.sizeof(_lib.HullCall) == 4 + 4 * 4 + 4 + 5 * 8              # (4 bytes of padding before the pointers)
    assert uaps_amd.hull_descriptors is hull.hull_descriptors and uaps_amd.HullResult is hull.HullResult
    assert uaps_amd.HULL_COLUMNS == R.COLUMNS


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.HullCall()
    c.struct_size = C.sizeof(_lib.HullCall)
    c.B, c.H, c.W, c.max_instances = 1, 8, 8, 4
    c.labels, c.table, c.workspace, c.workspace_bytes = 4096, 8192, 65536, 1 << 20       # never dereferenced: every call returns before a launch
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    run = lambda c: L.uaps_hull_descriptors(C.byref(c))
    assert L.uaps_hull_descriptors(None) == EINVAL
    assert run(_call(labels=None)) == EINVAL and run(_call(table=None)) == EINVAL and run(_call(workspace=None)) == EINVAL
    assert run(_call(table=4096)) == EINVAL                                                 # table == labels
    for dim in ("B", "H", "W"):
        assert run(_call(**{dim: 0})) == EINVAL and run(_call(**{dim: -3})) == EINVAL
    assert run(_call(max_instances=0)) == EINVAL and run(_call(max_instances=-1)) == EINVAL
    assert run(_call(struct_size=C.sizeof(_lib.HullCall) - 8)) == EINVAL                    # a header without `stream`
    assert run(_call(H=4097)) == ERANGE and run(_call(W=4097)) == ERANGE
    assert run(_call(B=16, H=4096, W=4096)) == ERANGE                                       # B * H * W * 8 = 2 GiB
    assert run(_call(B=4096, max_instances=3856)) == ERANGE                                 # a table of 2 GiB
    assert run(_call(B=1, H=4096, W=8, max_instances=65536)) == ERANGE                      # a workspace of 2 GiB
    need = C.c_size_t()
    assert L.uaps_hull_workspace_bytes(1, 8, 8, 4, C.byref(need)) == 0 and need.value == 4 * 9 * 8 + 224 and need.value % 256 == 0
    assert run(_call(workspace_bytes=need.value - 1)) == EWORKSPACE and run(_call(workspace=65536 + 128)) == EWORKSPACE
    assert L.uaps_hull_workspace_bytes(1, 8, 8, 4, None) == EINVAL and L.uaps_hull_workspace_bytes(0, 8, 8, 4, C.byref(need)) == EINVAL
    assert L.uaps_hull_workspace_bytes(1, 8, 8, 0, C.byref(need)) == EINVAL
    assert L.uaps_hull_workspace_bytes(1, 4097, 8, 4, C.byref(need)) == ERANGE
    assert L.uaps_hull_workspace_bytes(1, 4096, 8, 65536, C.byref(need)) == ERANGE


def test_census_the_hull_kernels():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    pattern = re.compile(r"^(?:void )?\(anonymous namespace\)::(hull_\w+(?:<[^>]*>)?)\(")
    built = norm_act_kernel_symbols(_lib.LIB_PATH, pattern)
    assert built == {"hull_zero_kernel", "hull_extents_kernel", "hull_measure_kernel"}, sorted(built)


# ---- inference.predict_instances(hull=...) ------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """Fixed logits: whatever the input, the arg-max is the label map the stub was built with."""

    def __init__(self, mask, classes):
        super().__init__()
        self.logits = torch.nn.functional.one_hot(torch.from_numpy(mask), classes).permute(0, 3, 1, 2).float() * 8.0

    def forward(self, x):
        return self.logits + 0.0 * x[:, :1]


def stub_mask():
    """Two images of classes 0..3: rims, a rim inside and a blob (hull_ref's rings), and noise."""
    return np.concatenate([R._rings(1, 37, 53), R._noise3(1, 37, 53)]).astype(np.int64)


def test_predict_instances_with_hull():
    from uaps_amd import HullResult, ShapeResult, SkeletonStats, hull_descriptors, inference, label_instances
    m = stub_mask()
    net = Stub(m, 4)
    x = torch.zeros(2, 3, 37, 53)
    plain = inference.predict_instances(net, x)
    assert isinstance(plain, type(label_instances(torch.from_numpy(m))))                    # unchanged without hull=
    assert isinstance(inference.predict_instances(net, x, hull=False), type(plain))
    h = inference.predict_instances(net, x, hull=True)
    assert isinstance(h, HullResult) and h.also is None and torch.equal(h.instances.labels, plain.labels)
    assert torch.equal(h.table, hull_descriptors(plain).table) and int(h.table[..., 0].sum()) > 0
    assert np.array_equal(h.table.numpy(), R.table(plain.labels.numpy(), 256))
    assert {"solidity", "feret_max", "rect_angle", "area"} <= set(h.records()[0][0])
    hs = inference.predict_instances(net, x, hull=True, shapes="thickness")
    assert isinstance(hs.also, ShapeResult) and hs.also.has_plane == "thickness" and torch.equal(hs.table, h.table)
    assert torch.equal(hs.also.table, inference.predict_instances(net, x, shapes="thickness").table)
    assert {"solidity", "inradius", "centroid_y", "area"} <= set(hs.records()[0][0])
    hk = inference.predict_instances(net, x, hull=True, skeleton=True)
    assert isinstance(hk.also, SkeletonStats) and hk.also.shapes is None and torch.equal(hk.table, h.table)
    both = inference.predict_instances(net, x, hull=True, skeleton=True, shapes=True)
    assert isinstance(both.also, SkeletonStats) and isinstance(both.also.shapes, ShapeResult)
    assert {"solidity", "length", "centroid_y", "area"} <= set(both.records()[1][0])
    for bad in ("x", 1, None, {"a": 1}):
        with pytest.raises(ValueError, match="predict_instances: hull is False or True"):
            inference.predict_instances(net, x, hull=bad)
