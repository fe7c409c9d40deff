"""Defect skeletons on the device (csrc/skeleton.hip) against the per-pixel table reference (tests/skeleton_ref.py), bit for bit: the
host shapes and fillings; 63 x 127 and 130 x 161 (rows one short of and beyond whole words, several bands); 3 x 600 (two 512-pixel
tiles across, so the halo words are used); 8 x 4096 (eight tiles across); every forced band height and sub-iteration count against
the chosen ones; the iteration cap and the per-image convergence flag; the label-map rule; a side stream, a garbage and a recycled
workspace; and the statistics in both flush forms against a brute-force loop."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import ndimage

import skeleton_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_cache = {}


def case(name, H, W, seed=0, max_iters=64):
    key = (name, H, W, seed, max_iters)
    if key not in _cache:
        m = R.filling(name, H, W, seed)
        cl = R.classes_of(name)
        _cache[key] = (m, cl) + R.thin(m, cl, 0, max_iters)
    return _cache[key]


def run(m, cl, num_classes=3, **kw):
    from uaps_amd import skeletonize
    r = skeletonize(torch.from_numpy(np.array(m)).to(DEV), num_classes, classes=cl, **kw)
    assert r.mask.is_cuda and r.mask.dtype == torch.int64 and r.mask.shape == m.shape
    assert r.converged.is_cuda and r.converged.dtype == torch.bool and r.converged.shape == (m.shape[0],)
    return r.mask.cpu().numpy(), r.converged.cpu().numpy()


def same(got, ref):
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (len(bad), bad[:4])


@pytest.mark.parametrize("name", R.FILLINGS)
@pytest.mark.parametrize("shape", R.SHAPES + ((63, 127), (130, 161)))
def test_device_equals_the_reference(shape, name):
    H, W = shape
    m, cl, ref, iters, fixed = case(name, H, W, max_iters=80)
    if min(H, W) >= 3:
        assert not np.array_equal(ref, m) and np.isin(ref, cl).any()
    assert fixed.all()
    got, conv = run(m, cl, max_iters=80)
    same(got, ref)
    assert conv.all()


@pytest.mark.parametrize("name", ("noise0.65", "noise0.9", "discs", "full", "two"))
@pytest.mark.parametrize("shape", ((3, 600), (8, 4096)))
def test_tiles_across_a_row(shape, name):
    H, W = shape
    m, cl, ref, iters, fixed = case(name, H, W)
    assert not np.array_equal(ref, m) and np.isin(ref, cl).any() and fixed.all()
    got, conv = run(m, cl)
    same(got, ref)
    assert conv.all()
    got, conv = run(m, cl, _sub_iters=64, _band_rows=1)                         # the halo word used to its last pixel
    same(got, ref)


def test_band_height_and_sub_iterations_do_not_change_the_bits():
    from uaps_amd.skeleton import band_rows
    m, cl, ref, iters, fixed = case("noise0.9", 130, 161, seed=1)
    assert int(iters[0]) == 30 and fixed.all()                                  # several launches at every S, several bands
    chosen = band_rows(130, 161, 1)
    assert 1 <= chosen < 130
    for band in (4, 8, 0):
        for S in (2, 6, 0):
            got, conv = run(m, cl, _band_rows=band, _sub_iters=S)
            same(got, ref)
            assert conv.all(), (band, S)
    for band, S in ((1, 64), (130, 64), (37, 10), (chosen, 8)):
        got, conv = run(m, cl, _band_rows=band, _sub_iters=S)
        same(got, ref)


def test_the_cap_and_the_convergence_flag():
    m, cl, ref64, iters, fixed = case("full", 130, 161, max_iters=64)
    assert int(iters[0]) == 64 and not fixed[0]                                 # the frame needs 65
    got, conv = run(m, cl)
    same(got, ref64)
    assert not conv[0]
    m, cl, ref, iters, fixed = case("full", 130, 161, max_iters=80)
    assert int(iters[0]) == 65 and fixed[0]
    got, conv = run(m, cl, max_iters=80)
    same(got, ref)
    assert conv[0]
    got, conv = run(m, cl, max_iters=65)                                        # the cap met exactly: a fixed point all the same
    same(got, ref)
    assert conv[0]
    got, conv = run(m, cl, max_iters=3, _sub_iters=4)                           # a last launch shorter than the others
    same(got, R.thin(m, cl, 0, 3)[0])
    assert not conv[0]
    sparse = R.filling("salt", 130, 161)
    both = np.concatenate([m, sparse])
    got, conv = run(both, cl)
    same(got[:1], ref64)
    same(got[1:], R.thin(sparse, cl, 0, 64)[0])
    assert conv.tolist() == [False, True]


def test_label_map_rule_on_the_device():
    """Eight classes at once (0..7 selected, an explicit background of 8), a class subset in any order, ignore labels (255, -7)
    and the value 8 itself passing through."""
    from uaps_amd import skeletonize
    rng = np.random.default_rng(5)
    m = np.kron(rng.integers(0, 9, size=(2, 7, 15)), np.ones((10, 10), dtype=np.int64)).astype(np.int64)    # 10 x 10 blocks of 0..8
    m[rng.random(m.shape) < 0.1] = 8
    m[:, :, 40] = 255
    m[:, 33] = -7
    t = torch.from_numpy(m).to(DEV)
    r8 = skeletonize(t, 8, classes=(0, 1, 2, 3, 4, 5, 6, 7), background=8)
    ref8 = R.thin(m, range(8), 8, 64)[0]
    assert not np.array_equal(ref8, m)
    same(r8.mask.cpu().numpy(), ref8)
    keep = ~np.isin(m, range(8))
    assert np.array_equal(ref8[keep], m[keep]) and (m[keep] == 255).any() and (m[keep] == -7).any() and (m[keep] == 8).any()
    sub = skeletonize(t, 8, classes=(5, 2))                                     # a subset, in any order; background 0
    ref_sub = R.thin(m, (2, 5), 0, 64)[0]
    same(sub.mask.cpu().numpy(), ref_sub)
    assert np.array_equal(ref_sub[~np.isin(m, (2, 5))], m[~np.isin(m, (2, 5))])
    assert bool(r8.converged.all()) and bool(sub.converged.all())


def _raw(mask, cl, ws, max_iters=64, stream=None):
    from uaps_amd import _lib
    B, H, W = mask.shape
    out, conv = torch.empty_like(mask), torch.full((B,), 77, dtype=torch.uint8, device=DEV)
    c = _lib.SkeletonCall()
    c.struct_size = C.sizeof(_lib.SkeletonCall)
    c.B, c.H, c.W, c.n_classes, c.background, c.max_iters = B, H, W, len(cl), 0, max_iters
    for i, v in enumerate(cl):
        c.classes[i] = v
    c.mask, c.out, c.converged, c.workspace, c.workspace_bytes = mask.data_ptr(), out.data_ptr(), conv.data_ptr(), ws.data_ptr(), ws.numel()
    c.stream = _lib.current_stream(DEV) if stream is None else stream
    _lib.check(_lib.lib().uaps_skeletonize(C.byref(c)), "uaps_skeletonize")
    return out, conv


def test_two_runs_a_side_stream_and_a_garbage_workspace_give_the_same_bits():
    from uaps_amd import _lib, skeletonize
    m, cl, ref, iters, fixed = case("two", 65, 129)
    t = torch.from_numpy(m).to(DEV)
    need = _lib.workspace_bytes("uaps_skeleton_workspace_bytes", 1, 65, 129, len(cl))
    ws = torch.full((need,), 0xff, dtype=torch.uint8, device=DEV)               # garbage: every bit set, "last launch" words huge
    a, ca = _raw(t, cl, ws)
    b, cb = _raw(t, cl, ws)                                                     # recycled: the previous planes are no part of the next
    other = torch.from_numpy(case("discs", 65, 129)[0]).to(DEV)
    o, co = _raw(other, (1, 2), ws)
    same(a.cpu().numpy(), ref)
    same(b.cpu().numpy(), ref)
    same(o.cpu().numpy(), case("discs", 65, 129)[2])
    assert ca.tolist() == [1] and cb.tolist() == [1] and co.tolist() == [1]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        s = skeletonize(t, 3, classes=cl)
    side.synchronize()
    same(s.mask.cpu().numpy(), ref)
    again = skeletonize(t, 3, classes=cl)
    assert torch.equal(again.mask, s.mask) and torch.equal(again.converged, s.converged)


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def _plane_for(shape, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(-50, 5000, size=shape, dtype=np.int64)
    p[rng.random(shape) < 0.05] = 2 ** 31 - 1
    p[rng.random(shape) < 0.05] = -2 ** 31
    return p.astype(np.int32)


def _stats_case(name, H, W):
    """(skeleton map, classes, labels with values outside [0, M] mixed in, plane), on the host."""
    from uaps_amd import label_instances
    m, cl, ref = case(name, H, W)[:3]
    labels = label_instances(torch.from_numpy(m), max_instances=4096).labels.numpy().copy()
    rng = np.random.default_rng(H + W)
    stray = rng.random(labels.shape) < 0.03
    labels[stray] = rng.choice(np.array([-1, -2 ** 31, 2 ** 31 - 1, 100000], dtype=np.int64), size=int(stray.sum())).astype(np.int32)
    return ref, cl, labels, _plane_for(m.shape, H * 131 + W)


def _device_stats(ref, cl, labels, plane, M):
    from uaps_amd import skeleton_descriptors, SkeletonResult
    from uaps_amd.instances import InstanceResult
    B = labels.shape[0]
    inst = InstanceResult(torch.from_numpy(labels).to(DEV), torch.zeros(B, dtype=torch.int32, device=DEV),
                          torch.zeros((B, M, 9), dtype=torch.int64, device=DEV), 0)
    skel = SkeletonResult(torch.from_numpy(ref).to(DEV), torch.ones(B, dtype=torch.bool, device=DEV), tuple(cl))
    with_plane = skeleton_descriptors(inst, skel, _plane=torch.from_numpy(plane).to(DEV))
    bare = skeleton_descriptors(inst, skel, thickness=False)
    assert with_plane.table.is_cuda and with_plane.table.dtype == torch.int64 and tuple(with_plane.table.shape) == (B, M, 7)
    return with_plane.table.cpu().numpy(), bare.table.cpu().numpy()


@pytest.mark.parametrize("name,H,W", (("noise0.65", 65, 129), ("two", 37, 53), ("discs", 130, 161), ("noise0.9", 3, 600), ("full", 1, 70),
                                      ("noise0.5", 2, 2), ("salt", 64, 64), ("noise0.35", 70, 1), ("noise0.5", 5, 1100)))
def test_statistics_equal_brute_force_in_both_flush_forms(name, H, W):
    ref, cl, labels, plane = _stats_case(name, H, W)
    got = {}
    for M in (1, 3, 256, 257):
        want = R.stats(labels, ref, cl, plane, M)
        got[M], bare = _device_stats(ref, cl, labels, plane, M)
        bad = np.argwhere(got[M] != want)
        assert len(bad) == 0, (M, bad[:4], got[M][tuple(bad[0][:2])], want[tuple(bad[0][:2])])
        want[..., 5:] = 0
        assert np.array_equal(bare, want)
    assert np.array_equal(got[257][:, :256], got[256]) and np.array_equal(got[3], got[256][:, :3])     # the two forms against each other
    if H * W > 100:
        assert got[256][..., 0].sum() > 0 and got[256][..., 1:5].sum() > 0


def test_statistics_on_a_garbage_table_and_twice():
    from uaps_amd import _lib
    ref, cl, labels, plane = _stats_case("noise0.65", 65, 129)
    lab, sk, pl = (torch.from_numpy(v).to(DEV) for v in (labels, ref, plane))
    for M in (256, 257):
        want = R.stats(labels, ref, cl, plane, M)
        for fill in (0x5a5a5a5a5a5a5a5a, -1, None):
            table = torch.full((1, M, 7), fill, dtype=torch.int64, device=DEV) if fill is not None else table.clone()
            c = _lib.SkeletonStatsCall()
            c.struct_size = C.sizeof(_lib.SkeletonStatsCall)
            c.B, c.H, c.W, c.max_instances, c.n_classes = 1, 65, 129, M, len(cl)
            for i, v in enumerate(cl):
                c.classes[i] = v
            c.labels, c.skel, c.plane, c.table, c.stream = lab.data_ptr(), sk.data_ptr(), pl.data_ptr(), table.data_ptr(), _lib.current_stream(DEV)
            _lib.check(_lib.lib().uaps_skeleton_stats(C.byref(c)), "uaps_skeleton_stats")
            assert np.array_equal(table.cpu().numpy(), want), (M, fill)


def test_thickness_equals_the_host_distance_transform():
    from uaps_amd import label_instances, skeletonize, skeleton_descriptors
    m, cl, ref = case("discs", 130, 161)[:3]
    t = torch.from_numpy(m).to(DEV)
    inst = label_instances(t, max_instances=64)
    skel = skeletonize(t, 3, classes=cl)
    st = skeleton_descriptors(inst, skel)
    labels = inst.labels.cpu().numpy()
    d2 = np.rint(ndimage.distance_transform_edt(labels[0] != 0) ** 2).astype(np.int64)[None]
    want = R.stats(labels, ref, cl, d2, 64)
    assert st.has_plane and np.array_equal(st.table.cpu().numpy(), want) and want[..., 5].max() > 1
    p = st.props()
    k = int(np.argmax(want[0, :, 0]))
    assert p["width_max"][0, k] == 2.0 * np.sqrt(want[0, k, 5]) - 1.0 and p["skeleton_pixels"][0, k] == want[0, k, 0]


class Stub(torch.nn.Module):
    def __init__(self, mask, classes):
        super().__init__()
        self.register_buffer("logits", torch.nn.functional.one_hot(torch.from_numpy(mask), classes).permute(0, 3, 1, 2).float() * 8.0)

    def forward(self, x):
        return self.logits + 0.0 * x[:, :1]


def test_predict_instances_on_the_device_equals_the_cpu_path():
    from uaps_amd import inference
    m = np.concatenate([R.filling("discs", 64, 64), R.filling("two", 64, 64)])
    m[m == 255] = 0
    cpu_net, x = Stub(m, 3), torch.zeros(2, 3, 64, 64)
    dev_net = Stub(m, 3).to(DEV)
    for kw in (dict(skeleton=True), dict(skeleton={"max_iters": 2}, shapes="thickness")):
        a = inference.predict_instances(cpu_net, x, **kw)
        b = inference.predict_instances(dev_net, x.to(DEV), **kw)
        assert b.table.is_cuda and torch.equal(a.table, b.table.cpu())                      # the integers: exact
        assert torch.equal(a.skeleton.mask, b.skeleton.mask.cpu()) and torch.equal(a.skeleton.converged, b.skeleton.converged.cpu())
        assert torch.equal(a.instances.labels, b.instances.labels.cpu()) and torch.equal(a.instances.table[..., :7], b.instances.table[..., :7].cpu())
        ra, rb = a.records(), b.records()
        assert len(ra) == len(rb) == 2 and [len(r) for r in ra] == [len(r) for r in rb] and len(ra[0]) > 0
        for qa, qb in zip(ra[0] + ra[1], rb[0] + rb[1]):
            assert set(qa) == set(qb)
            for key in ("label", "cls", "area", "bbox", "length", "endpoints", "branch_points", "width_mean", "width_max", "skeleton_pixels"):
                assert qa[key] == qb[key] or (qa[key] != qa[key] and qb[key] != qb[key]), key
