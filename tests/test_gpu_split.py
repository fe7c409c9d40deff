"""Splitting of touching defects on the device (csrc/split.hip) against the per-marker flood on scipy (tests/split_ref.py): the shape
table of the host tests bit for bit, frames around the tile extent, long chains that need hundreds of rounds, many launches and every
tile seam, every rounds-per-launch value and forced tiles, a recycled workspace, the trivial splits, the closed loop with
match_instances, the downstream calls and the split= keyword of inference.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import instances_ref as IR
import split_ref as R
from test_split_host import SHAPES, _maps, _run

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = 32                               # csrc/split.hip: kDefaultCols, rows and columns a tile owns (asserted below)
FRAMES = ((8, 4096), (4096, 8))


def _markers(mk):
    return torch.from_numpy(mk).to(DEV)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("form", ("distance", "markers"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_device_equals_the_reference(shape, form, connectivity):
    case = R.case(2, *shape, connectivity)
    for mma in (1, 4):
        ref = case.expected(form, min_marker_area=mma)                      # (asserts "informative" from 37 x 53 on)
        R.assert_equal(_run(case, form, DEV, min_marker_area=mma), ref, (shape, form, connectivity, mma))


@pytest.mark.parametrize("shape", FRAMES, ids=lambda s: "%dx%d" % s)
def test_device_equals_the_reference_on_long_frames(shape):
    case = R.case(1, *shape, 8)
    for form in ("distance", "markers"):
        R.assert_equal(_run(case, form, DEV), case.expected(form), (shape, form))
    assert (case.expected("markers")["pieces"] >= 2).any()


def test_frames_around_the_tile_extent():
    from uaps_amd.split import band_rows
    assert band_rows(256, 256) == (TILE, TILE) and band_rows(TILE, TILE + 1) == (TILE, TILE) and band_rows(5, 7) == (5, 7)
    cut = 0
    for e in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        for shape in ((e, 45), (45, e)):
            case = R.case(1, *shape, 8, seed=e)
            for form in ("distance", "markers"):
                ref = case.expected(form, check=False)                      # (one small image each: the claim is made of their sum)
                cut += int((ref["pieces"] >= 2).sum())
                R.assert_equal(_run(case, form, DEV), ref, (shape, form))
                R.assert_equal(_run(case, form, DEV, _band_rows=(TILE, TILE)), ref, (shape, form, "forced"))
    assert cut >= 4


@pytest.mark.parametrize("M", (1, 3, 256, 257))
def test_table_rows(M):
    case = R.case(2, 65, 129, 8)
    ref = case.expected("distance", max_instances=M)
    R.assert_equal(_run(case, "distance", DEV, max_instances=M), ref, M)
    assert ref["table"].shape[1] == M and (ref["count"] > 3).all()


@pytest.mark.parametrize("chain", ("spiral", "comb"))
@pytest.mark.parametrize("connectivity", (4, 8))
def test_long_chains_with_a_marker_at_each_end(chain, connectivity):
    """Hundreds of rounds, many launches, every tile seam: the fronts walk the chain from both ends and meet in the middle."""
    from uaps_amd import split_instances
    m = (IR.spiral if chain == "spiral" else IR.comb)(37, 53)
    ends = R.chain_ends(m)
    inst, labels, table = R.source(m, connectivity, DEV)
    assert int(inst.count[0]) == 1
    length = int((m != 0).sum())
    full = R.split_batch(labels, table, ends, connectivity=connectivity, max_iters=length)
    assert full["converged"].all() and full["count"][0] == 2
    res = split_instances(inst, markers=_markers(ends), connectivity=connectivity, max_iters=length)
    R.assert_equal(res, full, chain)
    third = length // 6                                                     # the fronts need about length / 2 rounds: a third of that
    cut = R.split_batch(labels, table, ends, connectivity=connectivity, max_iters=third)
    assert not cut["converged"].any() and cut["count"][0] == 3
    res = split_instances(inst, markers=_markers(ends), connectivity=connectivity, max_iters=third)
    R.assert_equal(res, cut, (chain, third))
    for S, rows in ((2, 0), (16, 0), (8, (8, 64)), (3, (16, 16))):
        R.assert_equal(split_instances(inst, markers=_markers(ends), connectivity=connectivity, max_iters=length, _sub_iters=S,
                                       _band_rows=rows), full, (chain, S, rows))


def test_a_front_crosses_a_tile_corner_diagonally():
    from uaps_amd import split_instances
    m = IR.diagonal(70, 70)                                                 # (31, 31) -> (32, 32): out of one tile into the one diagonally below
    mk = np.zeros(m.shape, dtype=bool)
    mk[0, 0, 0] = mk[0, 69, 69] = True
    inst, labels, table = R.source(m, 8, DEV)
    ref = R.split_batch(labels, table, mk)
    assert ref["count"][0] == 2 and ref["converged"].all() and ref["labels"][0, 34, 34] == 1 and ref["labels"][0, 35, 35] == 2
    for S in (0, 2, 16):
        for rows in (0, (TILE, TILE), (16, 16)):
            R.assert_equal(split_instances(inst, markers=_markers(mk), _sub_iters=S, _band_rows=rows), ref, (S, rows))
    lone = np.zeros(m.shape, dtype=bool)
    lone[0, 0, 0] = True                                                    # one marker: 69 rounds through every corner on the way
    ref = R.split_batch(labels, table, lone, max_iters=69)
    assert ref["converged"].all()
    R.assert_equal(split_instances(inst, markers=_markers(lone), max_iters=69), ref)
    short = R.split_batch(labels, table, lone, max_iters=33)                # stopped one pixel behind the corner
    assert not short["converged"].any() and short["count"][0] == 2
    R.assert_equal(split_instances(inst, markers=_markers(lone), max_iters=33), short)


def test_every_rounds_per_launch_value_and_forced_tiles_give_the_same_bits():
    for connectivity in (4, 8):
        case = R.case(2, 65, 129, connectivity)
        for form in ("distance", "markers"):
            ref = case.expected(form)
            for S in (2, 8, 16, 1, 5):
                for rows in (0, (16, 16), (8, 64)):
                    R.assert_equal(_run(case, form, DEV, _sub_iters=S, _band_rows=rows), ref, (form, S, rows))
            R.assert_equal(_run(case, form, DEV, _band_rows=13), ref, (form, "rows alone"))


def test_a_recycled_workspace():
    """A dense 256 x 256 call leaves large area words, owners and 'changed' words behind; the small calls after it must not see them."""
    from uaps_amd import label_instances, split_instances
    dense = label_instances(torch.ones((2, 256, 256), dtype=torch.int64, device=DEV))
    res = split_instances(dense, radius=5)                                  # no background: every pixel is a marker pixel
    assert torch.equal(res.instances.labels, dense.labels) and res.converged.all() and res.pieces[:, 0].tolist() == [1, 1]
    for shape in ((16, 16), (37, 53)):
        for connectivity in (4, 8):
            case = R.case(2, *shape, connectivity)
            for form in ("distance", "markers"):
                R.assert_equal(_run(case, form, DEV, min_marker_area=4), case.expected(form, min_marker_area=4), (shape, form))


def test_two_runs_give_the_same_bits():
    case = R.case(2, 65, 129, 8)
    a, b = _run(case, "distance", DEV), _run(case, "distance", DEV)
    for x, y in zip(tuple(a.instances[:3]) + tuple(a[1:4]), tuple(b.instances[:3]) + tuple(b[1:4])):
        assert torch.equal(x, y)


def test_trivial_splits_return_the_source():
    from uaps_amd import label_instances, split_instances
    case = R.case(2, 65, 129, 8)
    maps = _maps(case, DEV)
    inst = label_instances(torch.from_numpy(case.mask).to(DEV), maps)
    n = inst.count.cpu().numpy()
    for how in ({"radius": 100.0}, {"markers": torch.ones(case.mask.shape, dtype=torch.bool, device=DEV)},
                {"markers": torch.full(case.mask.shape, 7, dtype=torch.uint8, device=DEV)}):
        res = split_instances(inst, maps=maps, **how)                       # nothing has a marker / every defect is one marker
        for a, b in zip(res.instances[:3], inst[:3]):
            assert torch.equal(a, b)
        assert res.instances.n_maps == 2 and res.converged.all()
        parent, pieces = res.parent.cpu().numpy(), res.pieces.cpu().numpy()
        for b in range(2):
            assert parent[b, :n[b]].tolist() == list(range(1, n[b] + 1)) and (parent[b, n[b]:] == 0).all()
            assert (pieces[b, :n[b]] == 1).all() and (pieces[b, n[b]:] == 0).all()


def test_the_closed_loop_with_match_instances_and_the_downstream_calls():
    from uaps_amd import contours, match_instances, shape_descriptors
    case = R.case(2, 65, 129, 8)
    res = _run(case, "distance", DEV)
    src = case.inst(DEV)
    match = match_instances(res.instances, src, 4)
    t, parent = res.instances.table.cpu().numpy(), res.parent.cpu().numpy()
    got = match.pred.cpu().numpy()
    for b in range(2):
        n = int(res.instances.count[b])
        assert n > int(src.count[b])
        assert np.array_equal(got[b, :n, 0], parent[b, :n])                # every piece lies inside exactly one source: its parent
        assert np.array_equal(got[b, :n, 1], t[b, :n, 1]) and np.array_equal(got[b, :n, 2], t[b, :n, 1])
    shapes = shape_descriptors(res.instances, thickness=True)
    assert shapes.has_plane == "thickness" and (shapes.table.cpu().numpy()[..., 9][t[..., 1] > 0] >= 1).all()   # an inradius for every piece
    rings = contours(res.instances)
    outer = rings.summary.cpu().numpy()
    assert (outer[..., 0][t[..., 1] > 0] >= 1).all()                        # a ring for every piece


def _stub():
    from test_morph_host import Stub, _batches
    x = _batches(Stub(3, 4), 1)[0][0]
    return Stub(3, 4, heads=2).to(DEV), x.to(DEV)


def _against_reference(res, mask, maps, radius, connectivity=8, min_area=1):
    src, labels, table = R.source(mask.cpu().numpy(), connectivity, min_area=min_area)      # (the call's min_area is the source's too)
    d2 = int(np.ceil(radius * radius))
    ref = R.split_batch(labels, table, R.distance_sq(labels) >= d2, [m.cpu().numpy() for m in maps], connectivity, min_area=min_area)
    R.assert_equal(res.split._replace(instances=res), ref)
    assert torch.equal(res.split.source.labels.cpu(), src.labels)
    return ref


def test_predict_instances_with_split_on_the_device():
    from uaps_amd import consistency, inference
    from uaps_amd.tiled import predict_tiled
    from uaps_amd.tta import predict_tta
    net, x = _stub()
    with torch.no_grad():
        main, aux = net(x)
    unc = consistency.uncertainty_map(main, aux)
    mask = inference.predict(net, x)[0]
    res = inference.predict_instances(net, x, split=1.5)
    ref = _against_reference(res, mask, (torch.softmax(main, dim=1).amax(dim=1), unc), 1.5)
    assert (ref["pieces"] >= 2).any()
    res = inference.predict_instances(net, x, split={"radius": 1.5, "min_marker_area": 1, "max_iters": 64}, connectivity=4, min_area=2)
    _against_reference(res, mask, (torch.softmax(main, dim=1).amax(dim=1), unc), 1.5, 4, 2)
    t = predict_tta(net, x, scales=(1.0,), want=("mask", "conf"))
    res = inference.predict_instances(net, x, tta=(1.0,), split=1.5)
    _against_reference(res, t.mask, (t.conf, unc), 1.5)
    tl = predict_tiled(net, x, tile=16, overlap=4, uncertainty="auto", want=("mask", "conf"))
    res = inference.predict_instances(net, x, tiled={"tile": 16, "overlap": 4}, split=1.5)
    ref = _against_reference(res, tl.mask, (tl.conf,) + tuple(tl.maps), 1.5)
    assert (ref["pieces"] >= 2).any()
    shaped = inference.predict_instances(net, x, split=1.5, shapes=True, hull=True)
    assert torch.equal(shaped.also.instances.labels, inference.predict_instances(net, x, split=1.5).labels)


class _Blob(torch.nn.Module):
    """Two classes from the first input channel: class 1 where it is positive."""

    def forward(self, x):
        return torch.cat([-x[:, :1], x[:, :1]], dim=1) * 8.0


def test_evaluate_with_split_finds_both_discs_of_a_blob():
    from uaps_amd import inference
    y, x = np.mgrid[0:40, 0:48]
    left, right = (y - 20) ** 2 + (x - 14) ** 2 <= 64, (y - 20) ** 2 + (x - 33) ** 2 <= 64
    target = (left | right).astype(np.int64)                                # two discs of radius 8, three columns apart
    assert IR.label_batch(target[None])[1][0] == 2
    blob = left | right | ((abs(y - 20) <= 2) & (x >= 14) & (x <= 33))      # the prediction joins them through a neck
    image = torch.from_numpy(np.where(blob, 1.0, -1.0).astype(np.float32))[None, None].repeat(1, 3, 1, 1).to(DEV)
    batches = [(image, torch.from_numpy(target)[None].to(DEV))]
    plain = inference.evaluate(_Blob(), batches, instances=True)
    cut = inference.evaluate(_Blob(), batches, instances=True, split=5.0)
    assert plain["defects_pred"] == 1 and cut["defects_pred"] == 2 and plain["defects_gt"] == cut["defects_gt"] == 2
    assert plain["DefectRecall(%)"] == 0.0 and cut["DefectRecall(%)"] == 100.0
    assert all(cut[k] == plain[k] for k in ("mIoU(%)", "mDice(%)", "Accuracy(%)", "images"))
