"""Shape descriptors without a GPU: the package's CPU restatement (uaps_amd/shapes.py) against the brute-force reference
(tests/shapes_ref.py) bit for bit on the case table, the three bit-quad identities on every row, props() on analytic shapes and against
direct central moments, the wrapper's and the C ABI's argument checks (they return before any launch), and the kernel census."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import shapes_ref as R
from conftest import ROOT
from test_bn_ref import norm_act_kernel_symbols

EINVAL, ERANGE = -1, -2
EPS = 2.0 ** -53


def _inst(case, M):
    from uaps_amd.instances import InstanceResult
    labels, count, table = case.instances(M)
    return InstanceResult(torch.from_numpy(labels), torch.from_numpy(count), torch.from_numpy(table), 0)


def _from_mask(mask, connectivity=8, M=16, **kw):
    """shape_descriptors of the package's own CPU labelling of an int64 [H,W] or [B,H,W] mask."""
    from uaps_amd import label_instances, shape_descriptors
    m = torch.from_numpy(np.asarray(mask, dtype=np.int64))
    m = m if m.dim() == 3 else m[None]
    inst = label_instances(m, connectivity=connectivity, max_instances=M)
    return shape_descriptors(inst, connectivity=connectivity, **kw)


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_cpu_path_equals_the_reference_and_the_identities_hold(cid):
    from uaps_amd import shape_descriptors
    case = R.case(cid)
    for M in R.MS:
        inst = _inst(case, M)
        for with_plane in (False, True):
            res = shape_descriptors(inst, torch.from_numpy(case.plane) if with_plane else None, connectivity=case.connectivity)
            assert res.table.dtype == torch.int64 and tuple(res.table.shape) == (case.mask.shape[0], M, 11)
            assert np.array_equal(res.table.numpy(), case.table(M, with_plane)), (cid, M, with_plane)
        _identities(case, M, case.table(M, False))


def _identities(case, M, t):
    labels, count, itab = case.instances(M)
    area = itab[..., 1]
    q1, q2, q3, qd = (t[..., c] for c in (5, 6, 7, 8))
    q4x4 = 4 * area - (q1 + 2 * q2 + 3 * q3 + 2 * qd)
    assert (q4x4 >= 0).all() and (q4x4 % 4 == 0).all()
    e4 = q1 - q3 + (2 * qd if case.connectivity == 4 else -2 * qd)
    assert (e4 % 4 == 0).all()
    assert ((t == 0).all(axis=-1) == (area == 0)).all()                 # a row is zero exactly where there is no component
    for b in range(labels.shape[0]):
        for k in range(1, min(M, int(count[b])) + 1):
            P = labels[b] == k
            assert q1[b, k - 1] + q2[b, k - 1] + q3[b, k - 1] + 2 * qd[b, k - 1] == R.crack_perimeter(P), (case.id, b, k)
            assert 1 - e4[b, k - 1] // 4 == R.holes(P, case.connectivity), (case.id, b, k)


def test_the_case_table_is_informative():
    ids = R.CASE_IDS
    assert len(ids) == len(set(ids))
    seen = np.zeros(11, dtype=bool)
    for cid in ids:
        seen |= (R.case(cid).table(R.LDS_ROWS, True) != 0).any(axis=(0, 1))
    assert seen.all()                                                   # every column is non-zero somewhere
    over = [cid for cid in ids if int(R.case(cid).instances(3)[1].max()) > R.MS[-1]]
    assert any(c.startswith("checker4") for c in over)                  # far more components than rows
    assert R.case("full-1x2x2100").mask.shape[2] > 2 * 16 * 64          # crosses the carried span twice
    c = R.case("full-3x17x129")
    lab = c.instances(3)[0]
    assert lab[0, -1, -1] == lab[1, 0, 0] == 1                          # the same number at the end of one image and the start of the next
    assert (R.case("touch-3x17x129").instances(3)[1] > 3).all()


def _one(res, name, b=0, k=0):
    return float(res.props()[name][b, k])


def test_props_of_a_rectangle():
    for a, b, y0, x0 in ((3, 7, 2, 5), (8, 2, 0, 0), (5, 5, 1, 1), (1, 9, 4, 0)):
        m = np.zeros((a + y0 + 2, b + x0 + 3), dtype=np.int64)
        m[y0:y0 + a, x0:x0 + b] = 2
        res = _from_mask(m)
        p = {k: float(v[0, 0]) for k, v in res.props().items()}
        assert np.isnan(res.props()["centroid_y"][0, 1])
        assert p["centroid_y"] == pytest.approx(y0 + (a - 1) / 2, rel=1e-12) and p["centroid_x"] == pytest.approx(x0 + (b - 1) / 2, rel=1e-12)
        assert p["var_x"] == pytest.approx((b * b - 1) / 12, rel=1e-12) and p["var_y"] == pytest.approx((a * a - 1) / 12, rel=1e-12)
        assert p["cov_xy"] == 0.0 and p["holes"] == 0.0 and p["euler"] == 1.0 and p["extent"] == 1.0
        assert p["orientation"] == (0.0 if b >= a else pytest.approx(math.pi / 2, rel=1e-12))
        assert p["l1"] == pytest.approx((max(a, b) ** 2 - 1) / 12, rel=1e-12) and p["l2"] == pytest.approx((min(a, b) ** 2 - 1) / 12, rel=1e-12, abs=0.0)
        assert p["major_axis"] == pytest.approx(4 * math.sqrt((max(a, b) ** 2 - 1) / 12), rel=1e-12)
        assert p["perimeter_crack"] == 2 * (a + b) and p["equivalent_diameter"] == pytest.approx(math.sqrt(4 * a * b / math.pi), rel=1e-12)
        q2 = 2 * (a - 1) + 2 * (b - 1)
        assert p["perimeter"] == pytest.approx(q2 + 4 / math.sqrt(2), rel=1e-12)
        assert p["compactness"] == pytest.approx(4 * math.pi * a * b / (q2 + 4 / math.sqrt(2)) ** 2, rel=1e-12)


def test_props_of_diagonals_a_plus_a_square_and_one_pixel():
    n = 9
    for flip, want in ((False, math.pi / 4), (True, -math.pi / 4)):
        m = np.eye(n, dtype=np.int64)
        res = _from_mask(m[:, ::-1].copy() if flip else m)
        assert _one(res, "orientation") == pytest.approx(want, rel=1e-12)
        assert _one(res, "minor_axis") == 0.0 and _one(res, "l2") == 0.0 and _one(res, "eccentricity") == 1.0
        assert _one(res, "l1") == pytest.approx(2 * (n * n - 1) / 12, rel=1e-12) and _one(res, "holes") == 0.0
        assert _one(res, "perimeter_crack") == 4 * n
    plus = np.zeros((9, 9), dtype=np.int64)
    plus[4, 1:8] = plus[1:8, 4] = 1
    square = np.zeros((9, 9), dtype=np.int64)
    square[2:6, 3:7] = 1
    for m in (plus, square):
        res = _from_mask(m)
        assert _one(res, "l1") > 0 and _one(res, "l2") == pytest.approx(_one(res, "l1"), rel=1e-12) and _one(res, "orientation") == 0.0
        assert _one(res, "eccentricity") < 1e-7 and _one(res, "minor_axis") == pytest.approx(_one(res, "major_axis"), rel=1e-12)
    dot = np.zeros((3, 4), dtype=np.int64)
    dot[1, 2] = 3
    res = _from_mask(dot)
    p = {k: float(v[0, 0]) for k, v in res.props().items()}
    assert (p["centroid_y"], p["centroid_x"], p["l1"], p["l2"], p["major_axis"], p["eccentricity"], p["orientation"]) == (1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert p["perimeter_crack"] == 4.0 and p["perimeter"] == pytest.approx(4 / math.sqrt(2), rel=1e-12) and p["holes"] == 0.0 and p["extent"] == 1.0
    assert res.table[0, 0].tolist() == [1, 2, 1, 2, 4, 4, 0, 0, 0, 0, 0]


def test_props_of_rings():
    ring = np.zeros((9, 11), dtype=np.int64)
    ring[2:7, 3:9] = 1
    ring[3:6, 4:8] = 0
    for connectivity in (4, 8):
        res = _from_mask(ring, connectivity)
        assert _one(res, "holes") == 1.0 and _one(res, "euler") == 0.0 and _one(res, "extent") == pytest.approx(18 / 30, rel=1e-12)
        assert _one(res, "centroid_y") == 4.0 and _one(res, "centroid_x") == 5.5
    import components_ref as CR
    nested = np.minimum(CR.nested_rings(), 1)                           # two rings, one class: two components, one hole each
    res = _from_mask(nested, 4)
    assert res.instances.count.tolist() == [2] and _one(res, "holes", k=0) == 1.0 and _one(res, "holes", k=1) == 1.0
    joined = nested.copy()
    joined[0, 10, 2:8] = 1                                              # a bridge: ONE label under 4-connectivity; the gap between
    res = _from_mask(joined, 4)                                         # the rings, cut once, is still one hole: two holes
    assert res.instances.count.tolist() == [1] and _one(res, "holes") == 2.0 == R.holes(joined[0] == 1, 4)


def test_props_against_direct_central_moments():
    """The bar is the REFERENCE's cancellation: 64 eps l1, absolute, on l1, l2 and the variances."""
    worst = {k: 0.0 for k in ("var_x", "var_y", "cov_xy", "l1", "l2")}
    checked = 0
    for cid in R.CASE_IDS:
        case = R.case(cid)
        M = R.LDS_ROWS
        labels, count, _ = case.instances(M)
        from uaps_amd import shape_descriptors
        p = shape_descriptors(_inst(case, M), connectivity=case.connectivity).props()
        for b in range(labels.shape[0]):
            for k in range(1, min(M, int(count[b])) + 1):
                ref = R.central(labels[b] == k)
                bar = 64 * EPS * ref["l1"]
                for name in worst:
                    err = abs(p[name][b, k - 1] - ref[name])
                    assert err <= bar, (cid, b, k, name, err, bar)
                    if ref["l1"] > 0:
                        worst[name] = max(worst[name], err / (EPS * ref["l1"]))
                assert p["centroid_x"][b, k - 1] == pytest.approx(ref["centroid_x"], rel=1e-12, abs=1e-12)
                assert p["centroid_y"][b, k - 1] == pytest.approx(ref["centroid_y"], rel=1e-12, abs=1e-12)
                checked += 1
    assert checked > 2000
    print("max |props - direct| / (eps l1):", worst, "bar 64")
    recorded = open(os.path.join(ROOT, "profiles", "shapes_forms_tau.txt")).read()
    assert "64" in recorded and all(name in recorded for name in worst)


def test_thickness_and_plane_on_the_cpu():
    from scipy import ndimage
    from uaps_amd import label_instances, shape_descriptors
    case = R.case("rings-3x17x129")
    inst = label_instances(torch.from_numpy(case.mask), connectivity=4, max_instances=64)
    res = shape_descriptors(inst, thickness=True, connectivity=4)
    lab = inst.labels.numpy()
    p = res.props()
    assert res.has_plane == "thickness" and {"plane_max", "plane_mean", "inradius"} <= set(p)
    for b in range(lab.shape[0]):
        d2 = np.rint(ndimage.distance_transform_edt(lab[b] != 0) ** 2).astype(np.int64)
        for k in range(1, min(64, int(inst.count[b])) + 1):
            assert int(res.table[b, k - 1, 9]) == d2[lab[b] == k].max() and int(res.table[b, k - 1, 10]) == d2[lab[b] == k].sum()
            assert p["inradius"][b, k - 1] == math.sqrt(d2[lab[b] == k].max())
    recs = res.records()
    assert len(recs) == 3 and recs[0][0]["label"] == 1 and recs[0][0]["area"] == int(inst.table[0, 0, 1])
    assert recs[0][0]["inradius"] == p["inradius"][0, 0] and {"centroid_x", "holes", "perimeter"} <= set(recs[0][0])
    plain = shape_descriptors(inst, connectivity=4)
    assert plain.has_plane == "none" and "plane_max" not in plain.props() and (plain.table[..., 9:] == 0).all()


def test_argument_checks():
    from uaps_amd import label_instances, shape_descriptors
    from uaps_amd.instances import InstanceResult
    inst = label_instances(torch.ones(1, 4, 4, dtype=torch.int64))
    assert shape_descriptors(inst).table.shape == (1, 256, 11)
    plane = torch.zeros(1, 4, 4, dtype=torch.int32)
    for bad in (inst.labels, (inst.labels, inst.count, inst.table), None):
        with pytest.raises(TypeError):
            shape_descriptors(bad)
    with pytest.raises(TypeError):
        shape_descriptors(InstanceResult(inst.labels.long(), inst.count, inst.table))
    with pytest.raises(TypeError):
        shape_descriptors(InstanceResult(inst.labels[0], inst.count, inst.table))
    for p in (plane.long(), plane[0], plane.float(), torch.zeros(1, 4, 5, dtype=torch.int32), np.zeros((1, 4, 4), np.int32)):
        with pytest.raises(TypeError):
            shape_descriptors(inst, p)
    with pytest.raises(ValueError):
        shape_descriptors(inst, connectivity=6)
    with pytest.raises(ValueError):
        shape_descriptors(inst, plane, thickness=True)
    with pytest.raises(ValueError):
        shape_descriptors(InstanceResult(torch.zeros(1, 1, 16385, dtype=torch.int32), inst.count, inst.table))
    with pytest.raises(ValueError):
        shape_descriptors(InstanceResult(torch.zeros(1, 0, 4, dtype=torch.int32), inst.count, inst.table))


def test_header_signatures_and_library_agree_on_the_new_symbol():
    from uaps_amd import _lib, shapes
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert "uaps_shape_descriptors" in declared and "uaps_shape_descriptors" in _lib.SIGNATURES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "uaps_shape_descriptors")
    assert _lib.lib().uaps_abi_version() == 3
    body = re.search(r"typedef struct uaps_shape_call \{(.*?)\} uaps_shape_call;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.ShapeCall._fields_], names
    defines = dict(re.findall(r"#define (UAPS_SHAPE_[A-Z_]+) (\d+)", text))
    assert int(defines["UAPS_SHAPE_COLUMNS"]) == _lib.SHAPE_COLUMNS == len(shapes.SHAPE_COLUMNS) == 11 and shapes.SHAPE_COLUMNS == R.COLUMNS
    assert int(defines["UAPS_SHAPE_MAX_EXTENT"]) == _lib.SHAPE_MAX_EXTENT == 16384
    assert int(defines["UAPS_SHAPE_LDS_ROWS"]) == _lib.SHAPE_LDS_ROWS == R.LDS_ROWS
    assert C.sizeof(_lib.ShapeCall) == 4 + 4 * 4 + 4 + 4 * 8             # (4 bytes of padding before the pointers)


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.ShapeCall()
    c.struct_size = C.sizeof(_lib.ShapeCall)
    c.B, c.H, c.W, c.max_instances = 1, 8, 8, 4
    c.labels, c.plane, c.table = 4096, None, 8192                       # never dereferenced: every call returns before a launch
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    run = lambda c: L.uaps_shape_descriptors(C.byref(c))
    assert L.uaps_shape_descriptors(None) == EINVAL
    assert run(_call(labels=None)) == EINVAL and run(_call(table=None)) == EINVAL
    assert run(_call(table=4096)) == EINVAL                                                 # table == labels
    for dim in ("B", "H", "W"):
        assert run(_call(**{dim: 0})) == EINVAL and run(_call(**{dim: -3})) == EINVAL
    assert run(_call(max_instances=0)) == EINVAL and run(_call(max_instances=-1)) == EINVAL
    assert run(_call(struct_size=C.sizeof(_lib.ShapeCall) - 8)) == EINVAL                   # a header without `stream`
    assert run(_call(H=16385)) == ERANGE and run(_call(W=16385)) == ERANGE and run(_call(H=65536, W=32768)) == ERANGE
    assert run(_call(H=16384, W=16384)) == ERANGE                                           # B * H * W * 8 = 2 GiB
    assert run(_call(B=64, H=2048, W=2048)) == ERANGE
    assert run(_call(B=1024, max_instances=23832)) == ERANGE                                # a table of 2 GiB
    assert run(_call(B=4, max_instances=2 ** 23)) == ERANGE


def test_census_the_shape_kernels_are_those_the_cases_name():
    from uaps_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libuaps_hip.so is not built")
    pattern = re.compile(r"^(?:void )?\(anonymous namespace\)::(shape_\w+(?:<[^>]*>)?)\(")
    built = norm_act_kernel_symbols(_lib.LIB_PATH, pattern)
    assert built == set(R.KERNELS), (sorted(built), sorted(R.KERNELS))
