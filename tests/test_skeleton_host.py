"""Defect skeletons without a GPU: the package's CPU restatement (uaps_amd/skeleton.py) against the per-pixel table reference
(tests/skeleton_ref.py), bit for bit; topology checks of every result with scipy (no library thinning is installed, so these are the
real pin); the reference's iteration counts; the statistics against a brute-force loop; the C ABI's argument checks (they return
before any launch); and the skeleton= keyword of inference.predict_instances around a stub network.

The claim "the reference result differs from its input and is not empty" is asserted for every frame that has a 3 x 3 window; the
single-line shapes and 2 x 2 (where a noise or two-class filling may have nothing to thin) are compared without it, and 2 x 2 full
is pinned on its own below."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import skeleton_ref as R
from conftest import ROOT

EINVAL, ERANGE, EWORKSPACE = -1, -2, -3
EIGHT = np.ones((3, 3), dtype=bool)
_cache = {}


def case(name, H, W, seed=0, max_iters=64):
    """(input map, classes, reference map, iterations [1], fixed point [1]), computed once."""
    key = (name, H, W, seed, max_iters)
    if key not in _cache:
        m = R.filling(name, H, W, seed)
        cl = R.classes_of(name)
        _cache[key] = (m, cl) + R.thin(m, cl, 0, max_iters)
    return _cache[key]


def run(m, cl, **kw):
    from uaps_amd import skeletonize
    r = skeletonize(torch.from_numpy(np.array(m)), 3, classes=cl, **kw)
    assert r.mask.dtype == torch.int64 and r.mask.shape == m.shape and r.converged.dtype == torch.bool and r.converged.shape == (m.shape[0],)
    assert r.classes == tuple(cl) and r.background == 0
    return r


def holes(plane):
    """4-connected components of the zero-padded complement, minus the outside."""
    return ndimage.label(~np.pad(plane, 1))[1] - 1


def check_topology(before, after):
    assert not (after & ~before).any()                                          # a subset of the plane
    lab, n = ndimage.label(before, structure=EIGHT)
    lab2, n2 = ndimage.label(after, structure=EIGHT)
    assert n == n2
    for k in range(1, n + 1):                                                   # every component holds exactly one skeleton component
        inside = np.unique(lab2[(lab == k) & after])
        assert len(inside) == 1, (k, inside)
    assert holes(before) == holes(after)


@pytest.mark.parametrize("name", R.FILLINGS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_cpu_path_equals_reference_and_keeps_topology(shape, name):
    H, W = shape
    m, cl, ref, iters, fixed = case(name, H, W)
    if min(H, W) >= 3:
        assert not np.array_equal(ref, m) and np.isin(ref, cl).any()
    assert fixed.all()                                                          # 64 iterations suffice on these frames
    r = run(m, cl)
    assert np.array_equal(r.mask.numpy(), ref)
    assert bool(r.converged.all())
    for c in cl:
        check_topology(m[0] == c, ref[0] == c)
    others = ~np.isin(m, cl)
    assert np.array_equal(ref[others], m[others])                               # 0, 255: untouched
    again = run(ref, cl)                                                        # thinning the result again changes nothing
    assert np.array_equal(again.mask.numpy(), ref) and bool(again.converged.all())


def test_pixel_loop_and_table_lookup_agree():
    for H, W in ((2, 2), (3, 200), (37, 53)):
        for name in ("noise0.65", "full", "discs", "two"):
            m, cl = R.filling(name, H, W), R.classes_of(name)
            a, b = R.thin(m, cl, 0, 64), R.thin(m, cl, 0, 64, step=R.sub_iteration_pixels)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_reference_iteration_counts():
    m, cl, ref, iters, fixed = case("full", 2, 2)
    assert int((ref == 1).sum()) == 1 and int(iters[0]) == 1 and not np.array_equal(ref, m)
    m, cl, ref, iters, fixed = case("full", 37, 53)
    assert int((ref == 1).sum()) == 17 and int(iters[0]) == 18
    m, cl, ref, iters, fixed = case("noise0.9", 130, 161, seed=1)               # (the seed at which the reference takes 30)
    assert int(iters[0]) == 30 and fixed.all()
    for H, W in ((1, 70), (70, 1)):
        m, cl, ref, iters, fixed = case("full", H, W)
        assert int(iters[0]) == 0 and np.array_equal(ref, m)
    for args in (("full", 2, 2), ("full", 37, 53), ("noise0.9", 130, 161, 1)):
        m, cl, ref = case(*args)[:3]
        assert np.array_equal(run(m, cl).mask.numpy(), ref)


def test_cap_gives_the_reference_after_exactly_that_many_iterations():
    m, cl, ref, iters, fixed = case("full", 37, 53, max_iters=3)
    assert int(iters[0]) == 3 and not fixed[0]
    r = run(m, cl, max_iters=3)
    assert np.array_equal(r.mask.numpy(), ref) and not bool(r.converged[0]) and r.max_iters == 3
    # the cap met exactly: 18 iterations reach the fixed point of this frame, and the result is one
    full = case("full", 37, 53)[2]
    r = run(m, cl, max_iters=18)
    assert np.array_equal(r.mask.numpy(), full) and bool(r.converged[0])
    r = run(m, cl, max_iters=17)
    assert not np.array_equal(r.mask.numpy(), full) and not bool(r.converged[0])
    # a batch: per image
    sparse = np.zeros_like(m)
    sparse[0, 5, 3:40] = 1                                                      # a line: a skeleton already
    r = run(np.concatenate([m, sparse]), cl, max_iters=3)
    assert r.converged.tolist() == [False, True]


def test_label_map_rule():
    from uaps_amd import skeletonize
    m, cl, ref, _, _ = case("two", 37, 53)
    t = torch.from_numpy(m)
    only2 = skeletonize(t, 3, classes=[2]).mask.numpy()
    assert np.array_equal(only2, R.thin(m, (2,), 0, 64)[0]) and np.array_equal(only2[m == 1], m[m == 1])
    bg7 = skeletonize(t, 8, classes=[1, 2], background=7).mask.numpy()
    assert np.array_equal(bg7, R.thin(m, (1, 2), 7, 64)[0]) and (bg7 == 7).any() and np.array_equal(bg7 == 0, m == 0)
    default = skeletonize(t, 3).mask.numpy()                                    # all classes but the background
    assert np.array_equal(default, ref)
    assert (ref == 255).sum() == (m == 255).sum()


def test_wrapper_refuses_bad_arguments():
    from uaps_amd import skeletonize
    m = torch.ones(1, 8, 8, dtype=torch.int64)
    for bad in (m.int(), m[0], m.float()):
        with pytest.raises(TypeError):
            skeletonize(bad, 2)
    for kw in (dict(max_iters=0), dict(max_iters=2049), dict(max_iters=2.5), dict(classes=[0]), dict(classes=[1, 1]), dict(classes=[2]),
               dict(classes=[]), dict(_sub_iters=3), dict(_sub_iters=66), dict(_band_rows=-1), dict(background=2 ** 31)):
        with pytest.raises(ValueError):
            skeletonize(m, 2, **kw)
    with pytest.raises(ValueError):
        skeletonize(torch.zeros(1, 1, 4097, dtype=torch.int64), 2)
    with pytest.raises(ValueError):
        skeletonize(m, 9)


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def _instances(m, M):
    from uaps_amd import label_instances
    return label_instances(torch.from_numpy(m), max_instances=M)


def _plane_for(shape, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(-50, 5000, size=shape, dtype=np.int64)
    p[rng.random(shape) < 0.05] = 2 ** 31 - 1
    p[rng.random(shape) < 0.05] = -2 ** 31
    return p.astype(np.int32)


@pytest.mark.parametrize("M", (1, 3, 256, 257))
@pytest.mark.parametrize("name", R.FILLINGS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_statistics_equal_brute_force(shape, name, M):
    from uaps_amd import skeleton_descriptors, SkeletonResult, SKELETON_COLUMNS
    H, W = shape
    m, cl, ref = case(name, H, W)[:3]
    inst = _instances(m, M)
    skel = SkeletonResult(torch.from_numpy(ref), torch.ones(1, dtype=torch.bool), tuple(cl))
    plane = _plane_for(m.shape, H * 131 + W)
    want = R.stats(inst.labels.numpy(), ref, cl, plane, M)
    got = skeleton_descriptors(inst, skel, _plane=torch.from_numpy(plane))
    assert got.table.dtype == torch.int64 and got.table.shape == (1, M, len(SKELETON_COLUMNS)) and got.has_plane
    assert np.array_equal(got.table.numpy(), want)
    bare = skeleton_descriptors(inst, skel, thickness=False)
    want[..., 5:] = 0
    assert np.array_equal(bare.table.numpy(), want) and not bare.has_plane
    if min(H, W) >= 3 and M >= 3:
        assert want[..., 0].sum() > 0


def _figure(points, H=12, W=12):
    m = np.zeros((1, H, W), dtype=np.int64)
    for y, x in points:
        m[0, y, x] = 1
    return m


def _figure_stats(m, **kw):
    from uaps_amd import distance_transform_sq, skeleton_descriptors, SkeletonResult
    inst = _instances(m, 4)
    skel = SkeletonResult(torch.from_numpy(m), torch.ones(1, dtype=torch.bool), (1,))
    st = skeleton_descriptors(inst, skel, **kw)
    assert st.has_plane                                                         # thickness=True is the default
    assert np.array_equal(st.table.numpy(), R.stats(inst.labels.numpy(), m, (1,), distance_transform_sq(inst.labels).numpy(), 4))
    return dict(zip(("n_skel", "n_orth", "n_diag", "n_end", "n_branch", "d2max", "d2sum"), st.table[0, 0].tolist())), st


def test_fixed_figures():
    n = 9
    row, st = _figure_stats(_figure([(5, 1 + i) for i in range(n)]))
    assert (row["n_skel"], row["n_orth"], row["n_diag"], row["n_end"], row["n_branch"]) == (n, n - 1, 0, 2, 0)
    p = st.props()
    assert p["width_mean"][0, 0] == 1.0 and p["length"][0, 0] == n - 1 and p["endpoints"][0, 0] == 2 and p["branch_points"][0, 0] == 0
    assert p["width_max"][0, 0] == 1.0 and p["width_rms"][0, 0] == 1.0 and p["skeleton_pixels"][0, 0] == n
    assert np.isnan(p["length"][0, 1])
    row, st = _figure_stats(_figure([(1 + i, 1 + i) for i in range(n)]))
    assert (row["n_orth"], row["n_diag"], row["n_end"], row["n_branch"]) == (0, n - 1, 2, 0)
    assert st.props()["length"][0, 0] == math.sqrt(2.0) * (n - 1)
    stairs = [(1 + i // 2, 1 + (i + 1) // 2) for i in range(n)]                 # right, down, right, down ...
    row, _ = _figure_stats(_figure(stairs))
    assert (row["n_orth"], row["n_diag"]) == (n - 1, 0)                         # no corner is counted twice
    plus = [(5, x) for x in range(1, 10)] + [(y, 5) for y in range(1, 10) if y != 5]
    row, _ = _figure_stats(_figure(plus))
    assert row["n_end"] == 4 and row["n_branch"] >= 1 and row["n_orth"] == 16 and row["n_diag"] == 0
    ring = [(2, x) for x in range(2, 9)] + [(8, x) for x in range(2, 9)] + [(y, 2) for y in range(3, 8)] + [(y, 8) for y in range(3, 8)]
    row, _ = _figure_stats(_figure(ring))
    assert row["n_end"] == 0 and row["n_branch"] == 0 and row["n_orth"] == len(ring)
    row, st = _figure_stats(_figure([(4, 4)]))
    assert (row["n_skel"], row["n_orth"], row["n_diag"], row["n_end"], row["n_branch"]) == (1, 0, 0, 0, 0)
    assert st.props()["width_mean"][0, 0] == 1.0


def test_props_where_the_skeleton_was_cut_by_classes():
    from uaps_amd import skeleton_descriptors, SkeletonResult
    m = _figure([(5, 1 + i) for i in range(6)])
    m[0, 9, 2:8] = 2
    inst = _instances(m, 4)
    skel = SkeletonResult(torch.from_numpy(m), torch.ones(1, dtype=torch.bool), (1,))
    st = skeleton_descriptors(inst, skel)
    p = st.props()
    assert st.table[0, 1].tolist() == [0] * 7 and np.isnan(p["width_rms"][0, 1]) and p["length"][0, 1] == 0.0
    recs = st.records()
    assert len(recs[0]) == 2 and recs[0][0]["length"] == 5.0 and recs[0][0]["area"] == 6 and recs[0][1]["skeleton_pixels"] == 0.0


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def _fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*?\]", "", f).strip(" *") for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    return names


def test_header_signatures_and_library_agree_on_the_new_symbols():
    from uaps_amd import _lib
    new = {"uaps_skeletonize", "uaps_skeleton_workspace_bytes", "uaps_skeleton_band_rows", "uaps_skeleton_stats"}
    text = open(os.path.join(ROOT, "include", "uaps_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(uaps_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= set(_lib.SIGNATURES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(raw, n), n
    assert _lib.lib().uaps_abi_version() == 3
    assert _fields(hdr, "uaps_skeleton_call") == [f[0] for f in _lib.SkeletonCall._fields_]
    assert _fields(hdr, "uaps_skeleton_stats_call") == [f[0] for f in _lib.SkeletonStatsCall._fields_]
    defines = dict(re.findall(r"#define (UAPS_SKEL_[A-Z_]+) (\d+)", text))
    assert [int(defines["UAPS_SKEL_" + k]) for k in ("MAX_CLASSES", "MAX_ITERS", "MAX_SUB_ITERS", "MAX_EXTENT", "COLUMNS")] == \
        [_lib.SKEL_MAX_CLASSES, _lib.SKEL_MAX_ITERS, _lib.SKEL_MAX_SUB_ITERS, _lib.SKEL_MAX_EXTENT, _lib.SKEL_COLUMNS]
    assert C.sizeof(_lib.SkeletonCall) == 8 + 4 * 4 + 32 + 4 * 4 + 6 * 8
    assert C.sizeof(_lib.SkeletonStatsCall) == 4 + 5 * 4 + 32 + 5 * 8


def _call(**kw):
    from uaps_amd import _lib
    c = _lib.SkeletonCall()
    c.struct_size = C.sizeof(_lib.SkeletonCall)
    c.B, c.H, c.W, c.n_classes, c.background, c.max_iters, c.sub_iters, c.band_rows = 1, 8, 8, 2, 0, 64, 0, 0
    c.classes[0], c.classes[1] = 1, 2
    c.mask, c.out, c.converged, c.workspace, c.workspace_bytes = 4096, 8192, 12288, 16384, 1 << 20     # never dereferenced
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


def test_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()
    run_ = lambda c: L.uaps_skeletonize(C.byref(c))
    assert L.uaps_skeletonize(None) == EINVAL
    for p in ("mask", "out", "converged", "workspace"):
        assert run_(_call(**{p: None})) == EINVAL
    assert run_(_call(out=4096)) == EINVAL                                                  # out == mask
    for dim in ("B", "H", "W"):
        assert run_(_call(**{dim: 0})) == EINVAL and run_(_call(**{dim: -3})) == EINVAL
    assert run_(_call(n_classes=0)) == EINVAL and run_(_call(n_classes=9)) == EINVAL
    assert run_(_call(classes=[1, 1])) == EINVAL and run_(_call(classes=[1, 0])) == EINVAL and run_(_call(background=2)) == EINVAL
    assert run_(_call(max_iters=0)) == EINVAL and run_(_call(max_iters=2049)) == EINVAL
    for s in (-2, 1, 3, 65, 66):
        assert run_(_call(sub_iters=s)) == EINVAL
    assert run_(_call(band_rows=-1)) == EINVAL
    assert run_(_call(struct_size=C.sizeof(_lib.SkeletonCall) - 8)) == EINVAL              # a header without `stream`
    assert run_(_call(H=4097)) == ERANGE and run_(_call(W=4097)) == ERANGE
    assert run_(_call(B=64, H=2048, W=2048)) == ERANGE                                      # B * H * W * 8 = 2 GiB
    assert run_(_call(band_rows=4096)) == ERANGE                                            # planes that cannot fit
    assert run_(_call(workspace_bytes=64)) == EWORKSPACE and run_(_call(workspace=16384 + 8)) == EWORKSPACE
    need = C.c_size_t(0)
    assert L.uaps_skeleton_workspace_bytes(2, 130, 161, 3, C.byref(need)) == 0
    assert need.value >= 2 * 3 * 2 * 130 * 3 * 8 + 2 * 4 and need.value % 256 == 0
    assert L.uaps_skeleton_workspace_bytes(2, 130, 161, 3, None) == EINVAL and L.uaps_skeleton_workspace_bytes(0, 8, 8, 1, C.byref(need)) == EINVAL
    assert L.uaps_skeleton_workspace_bytes(1, 8, 8, 0, C.byref(need)) == EINVAL and L.uaps_skeleton_workspace_bytes(1, 8, 8, 9, C.byref(need)) == EINVAL
    assert L.uaps_skeleton_workspace_bytes(1, 4097, 8, 1, C.byref(need)) == ERANGE
    rows = C.c_int(-1)
    assert L.uaps_skeleton_band_rows(256, 256, 4, 0, C.byref(rows)) == 0 and 1 <= rows.value <= 256
    assert L.uaps_skeleton_band_rows(1, 1, 2, 2, C.byref(rows)) == 0 and rows.value == 1
    assert L.uaps_skeleton_band_rows(8, 8, 4, 2, None) == EINVAL and L.uaps_skeleton_band_rows(0, 8, 4, 2, C.byref(rows)) == EINVAL
    assert L.uaps_skeleton_band_rows(8, 8, 1, 2, C.byref(rows)) == EINVAL and L.uaps_skeleton_band_rows(8, 8, 10, 2, C.byref(rows)) == EINVAL
    assert L.uaps_skeleton_band_rows(8, 8, 4, 3, C.byref(rows)) == EINVAL and L.uaps_skeleton_band_rows(8, 8, 4, 66, C.byref(rows)) == EINVAL
    assert L.uaps_skeleton_band_rows(8, 4097, 4, 2, C.byref(rows)) == ERANGE
    # both copies of every staged tile the library chooses (band + 2 S rows of at most 8 + 2 words) fit 64 KiB
    for H, W, S in ((256, 256, 0), (1024, 1024, 8), (4096, 4096, 64), (130, 161, 2), (5, 4096, 32)):
        assert L.uaps_skeleton_band_rows(H, W, 9, S, C.byref(rows)) == 0
        assert 2 * (rows.value + 2 * (S or 8)) * 10 * 8 <= 65536 and 1 <= rows.value <= H, (H, W, S, rows.value)


def test_stats_c_abi_refuses_before_any_launch():
    from uaps_amd import _lib
    L = _lib.lib()

    def call(**kw):
        c = _lib.SkeletonStatsCall()
        c.struct_size = C.sizeof(_lib.SkeletonStatsCall)
        c.B, c.H, c.W, c.max_instances, c.n_classes = 1, 8, 8, 4, 1
        c.classes[0] = 1
        c.labels, c.skel, c.table = 4096, 8192, 12288
        for k, v in kw.items():
            setattr(c, k, v)
        return L.uaps_skeleton_stats(C.byref(c))
    assert L.uaps_skeleton_stats(None) == EINVAL
    for p in ("labels", "skel", "table"):
        assert call(**{p: None}) == EINVAL
    assert call(table=4096) == EINVAL and call(table=8192) == EINVAL
    for dim in ("B", "H", "W", "max_instances", "n_classes"):
        assert call(**{dim: 0}) == EINVAL
    assert call(n_classes=9) == EINVAL
    assert call(struct_size=C.sizeof(_lib.SkeletonStatsCall) - 8) == EINVAL
    assert call(H=16385) == ERANGE and call(W=16385) == ERANGE and call(B=64, H=2048, W=2048) == ERANGE
    assert call(B=4096, max_instances=16384) == ERANGE                                      # a table of 3.5 GiB


# ---- inference.predict_instances(skeleton=...) ------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """Fixed logits: whatever the input, the arg-max is the label map the stub was built with."""

    def __init__(self, mask, classes):
        super().__init__()
        self.logits = torch.nn.functional.one_hot(torch.from_numpy(mask), classes).permute(0, 3, 1, 2).float() * 8.0

    def forward(self, x):
        return self.logits + 0.0 * x[:, :1]


def test_predict_instances_with_skeleton():
    from uaps_amd import inference, label_instances, skeletonize, skeleton_descriptors, SkeletonStats
    m = np.concatenate([R.filling("discs", 37, 53), R.filling("two", 37, 53)])
    m[m == 255] = 0
    net = Stub(m, 3)
    x = torch.zeros(2, 3, 37, 53)
    plain = inference.predict_instances(net, x)
    assert isinstance(plain, type(label_instances(torch.from_numpy(m))))                    # unchanged without skeleton=
    assert torch.equal(plain.labels, label_instances(torch.from_numpy(m)).labels)
    st = inference.predict_instances(net, x, skeleton=True)
    assert isinstance(st, SkeletonStats) and st.shapes is None and st.has_plane
    skel = skeletonize(torch.from_numpy(m), 3)
    assert torch.equal(st.skeleton.mask, skel.mask) and torch.equal(st.instances.labels, plain.labels)
    assert torch.equal(st.table, skeleton_descriptors(plain, skel).table) and int(st.table[..., 0].sum()) > 0
    assert np.array_equal(st.skeleton.mask.numpy(), R.thin(m, (1, 2), 0, 64)[0])
    recs = st.records()
    assert len(recs[1]) == int(plain.count[1]) and {"length", "endpoints", "branch_points", "width_mean", "width_max", "width_rms"} <= set(recs[1][0])
    capped = inference.predict_instances(net, x, skeleton={"max_iters": 1})
    assert capped.skeleton.max_iters == 1 and not bool(capped.skeleton.converged.all())
    assert np.array_equal(capped.skeleton.mask.numpy(), R.thin(m, (1, 2), 0, 1)[0])
    both = inference.predict_instances(net, x, skeleton=True, shapes="thickness")
    assert isinstance(both, SkeletonStats) and both.shapes is not None and torch.equal(both.table, st.table)
    shp = inference.predict_instances(net, x, shapes="thickness")
    assert torch.equal(both.shapes.table, shp.table)
    merged = both.records()
    assert {"length", "inradius", "centroid_y", "area"} <= set(merged[0][0])
    clean = inference.predict_instances(net, x, skeleton=True, cleanup=[("open", "disk", 1)])
    from uaps_amd import morphology
    opened = morphology(torch.from_numpy(m), [("open", "disk", 1)], 3)
    assert torch.equal(clean.skeleton.mask, skeletonize(opened, 3).mask)
    for bad in (1, "yes", {"iters": 3}, None):
        with pytest.raises(ValueError):
            inference.predict_instances(net, x, skeleton=bad)
