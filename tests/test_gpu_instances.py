"""Defect instances and run-length masks on the GPU (csrc/instances.hip) against scipy (tests/instances_ref.py) and the reference's
strings (tests/golden/g13_rle.npz).  Every comparison is exact: integers, and bit-equal fixed-point sums.

The kernels label 16 x 16 tiles in LDS (instances_ref.TILE) and merge them along their seams: 37 x 53 is 3 x 4 tiles and 130 x 70 is
9 x 5, both ending in ragged tiles in both directions; 256 x 256 is 16 x 16 whole tiles, 7 x 300 one ragged row of 19."""
import os

import numpy as np
import pytest
import torch

import instances_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = R.DEV
SHAPES = ((1, 1, 1), (1, 1, 45), (1, 7, 300), (3, 37, 53), (2, 130, 70), (2, 256, 256))


def _patterns(B, H, W):
    """name -> int64 [B,H,W]: image 0 is the pattern, the others class noise (so that images must not leak into each other)."""
    out = {"noise": R.noise(B, H, W, 0.5, seed=H + W), "full": np.full((B, H, W), 2, dtype=np.int64), "empty": np.zeros((B, H, W), dtype=np.int64)}
    for name, fn in (("spiral", R.spiral), ("comb", R.comb), ("diagonal", R.diagonal), ("corners", R.corners)):
        m = R.noise(B, H, W, 0.4, seed=3 * H + W)
        m[0] = fn(H, W)[0]
        out[name] = m
    return out


def _run(m, maps, **kw):
    from uaps_amd import label_instances
    return label_instances(torch.from_numpy(m).to(DEV), [torch.from_numpy(v).to(DEV) for v in maps], **kw)


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_equals_scipy(shape, connectivity):
    B, H, W = shape
    maps = R.random_maps(B, H, W)
    for name, m in _patterns(B, H, W).items():
        res = _run(m, maps, connectivity=connectivity, max_instances=512)
        R.assert_equal(res, R.label_batch(m, maps, connectivity, 0, 1, 512), f"{name} {shape} c{connectivity}")
    # every class forms components, the background class included
    m = _patterns(B, H, W)["noise"]
    res = _run(m, maps[:1], connectivity=connectivity, background=None, max_instances=512)
    R.assert_equal(res, R.label_batch(m, maps[:1], connectivity, None, 1, 512), f"no background {shape}")
    assert res.n_maps == 1 and int(res.table[..., 8].abs().sum()) == 0


def test_diagonal_separates_the_connectivities():
    m = R.diagonal(130, 70)
    assert _run(m, (), connectivity=8).count.tolist() == [1] and _run(m, (), connectivity=4).count.tolist() == [70]


def test_checkerboard_overflow():
    m = R.checkerboard(37, 53)
    one = _run(m, (), connectivity=8)
    assert one.count.tolist() == [1] and one.table[0, 0, :7].tolist() == [1, 981, 0, 0, 37, 53, 0] and not bool(one.overflow.any())
    many = _run(m, (), connectivity=4, max_instances=256)
    assert many.count.tolist() == [981] and many.overflow.tolist() == [True]
    R.assert_equal(many, R.label_batch(m, (), 4, 0, 1, 256))
    assert int(many.labels.max()) == 981 and bool((many.table[0, :, 1] == 1).all()) and len(many.records()[0]) == 256


@pytest.mark.parametrize("min_area", (2, 5, 12))
def test_min_area_removes_the_reference_set_and_renumbers(min_area):
    m = R.noise(2, 130, 70, 0.45, seed=11)
    maps = R.random_maps(2, 130, 70)
    for connectivity in (4, 8):
        ref = R.label_batch(m, maps, connectivity, 0, min_area, 512)
        res = _run(m, maps, connectivity=connectivity, min_area=min_area, max_instances=512)
        R.assert_equal(res, ref, f"min_area {min_area}")
        assert int(res.count[0]) < int(_run(m, (), connectivity=connectivity, max_instances=512).count[0])      # (12 under 4-connectivity: none left)


def test_two_calls_same_bits_and_a_side_stream_with_recycled_workspace():
    m = R.noise(2, 130, 70, 0.5, seed=5)
    maps = R.random_maps(2, 130, 70)
    a, b = _run(m, maps, max_instances=512), _run(m, maps, max_instances=512)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = R.noise(2, 130, 70, 0.3, seed=6)
        first = _run(other, maps, max_instances=512)          # dirties this stream's workspace
        c = _run(m, maps, max_instances=512)                   # the same buffer again, not cleared in between
    side.synchronize()
    R.assert_equal(first, R.label_batch(other, maps, 8, 0, 1, 512))
    for x, y in zip(a[:3], c[:3]):
        assert torch.equal(x, y)


def test_clamp_rule_for_nan_and_huge_values():
    m = R.noise(1, 37, 53, 0.6, seed=2)
    v = R.random_maps(1, 37, 53)
    v[0][0, ::5, ::3] = np.nan
    v[0][0, 1::7, ::2] = 1e9
    v[1][0, ::4, 1::3] = -1e9
    v[1][0, 2::9] = np.inf
    res = _run(m, v, max_instances=1024)
    R.assert_equal(res, R.label_batch(m, v, 8, 0, 1, 1024))
    assert int(res.table[..., 7].abs().max()) >= 65536 * 2 ** 24
    mean = res.means()
    t = res.table[0, 0]
    assert float(mean[0, 0, 1]) == int(t[8]) / 16777216.0 / int(t[1])


def _golden():
    g = np.load(os.path.join(GOLDEN, "g13_rle.npz"))
    return [(str(n), g["mask_" + str(n)], str(g["rle_" + str(n)])) for n in g["names"]]


def test_rle_on_the_device_equals_the_reference_strings():
    from uaps_amd import format_rle, mask_to_rle, parse_rle, rle_to_mask
    for name, mask, text in _golden():                        # 200 x 200, 5 x 7, empty, full, single pixel, the last pixel, ...
        H, W = mask.shape
        dm = torch.from_numpy(mask.astype(np.int64))[None].to(DEV)
        rle = mask_to_rle(dm, (1,))
        assert rle.pairs.is_cuda and rle.pairs.dtype == torch.int32 and format_rle(rle.segment(0, 0)) == text, name
        assert rle.offsets.tolist() == [0, len(text.split()) // 2]
        back = rle_to_mask(parse_rle(text, (H, W)).to(DEV), rle.offsets, (H, W), (1,), dtype=torch.uint8)
        assert back.dtype == torch.uint8 and torch.equal(back, dm.to(torch.uint8)), name
        assert torch.equal(rle_to_mask(rle.pairs, rle.offsets, (H, W), (1,)), dm), name


@pytest.mark.parametrize("shape", ((1, 200, 200), (2, 5, 7), (2, 130, 70)), ids=lambda s: "x".join(map(str, s)))
def test_rle_round_trip_with_three_classes(shape):
    from uaps_amd import mask_to_rle, rle_to_mask
    B, H, W = shape
    m = R.class_mask(B, H, W)
    classes = (1, 2, 3)
    rle = mask_to_rle(torch.from_numpy(m).to(DEV), classes)
    pairs, off = rle.pairs.cpu().numpy(), rle.offsets.tolist()
    assert len(off) == B * 3 + 1 and off[0] == 0 and off[-1] == len(pairs)
    for b in range(B):
        for k, c in enumerate(classes):
            j = b * 3 + k
            assert np.array_equal(pairs[off[j]:off[j + 1]], R.mask2rle_pairs(m[b] == c)), (b, c)
    assert np.array_equal(rle_to_mask(rle.pairs, rle.offsets, (H, W), classes).cpu().numpy(), m)
    assert np.array_equal(rle_to_mask(rle.pairs, rle.offsets, (H, W), classes, dtype=torch.uint8).cpu().numpy(), m.astype(np.uint8))
    # the uint8 arrays the input pipelines keep encode to the same runs
    assert torch.equal(mask_to_rle(torch.from_numpy(m.astype(np.uint8)).to(DEV), classes).pairs, rle.pairs)
    # a segment's class is what the call names
    swapped = rle_to_mask(rle.pairs, rle.offsets, (H, W), (3, 2, 1)).cpu().numpy()
    assert np.array_equal(swapped, np.where(m == 1, 3, np.where(m == 3, 1, m)))


def test_rle_decode_later_classes_win_and_runs_need_no_order():
    from uaps_amd import rle_from_strings, rle_to_mask
    r = rle_from_strings([["3 4 1 2", "2 3"], ["", "9 1 1 9"]], (3, 3), (5, 9), device=DEV)
    flat = np.zeros((2, 9), dtype=np.int64)
    flat[0, 0:6] = 5; flat[0, 1:4] = 9; flat[1] = 9
    want = np.stack([f.reshape(3, 3, order="F") for f in flat])
    assert np.array_equal(rle_to_mask(r.pairs, r.offsets, (3, 3), (5, 9)).cpu().numpy(), want)


def test_predict_instances():
    import uaps_amd
    from uaps_amd import consistency, inference, label_instances
    torch.manual_seed(0)
    model = uaps_amd.net_factory("unet_uaps", 3, 4).to(DEV)
    x = torch.randn(2, 3, 64, 64, device=DEV)
    uaps_amd.perturb_manual_seed(7)
    res = inference.predict_instances(model, x, min_area=2, max_instances=512)
    uaps_amd.perturb_manual_seed(7)
    mask, heads = inference.predict(model, x)
    conf = torch.softmax(heads[0], dim=1).amax(dim=1)
    unc = consistency.uncertainty_map(heads[0], heads[1])
    want = label_instances(mask, (conf, unc), min_area=2, max_instances=512)
    assert res.n_maps == 2
    for a, b in zip(res[:3], want[:3]):
        assert torch.equal(a, b)
    R.assert_equal(res, R.label_batch(mask.cpu().numpy(), [conf.cpu().numpy(), unc.cpu().numpy()], 8, 0, 2, 512))
    recs = res.records()
    assert [len(r) for r in recs] == res.count.tolist() and all(0.0 < r["mean0"] <= 1.0 for rr in recs for r in rr)
    # with test-time augmentation: mask and confidence of predict_tta
    uaps_amd.perturb_manual_seed(7)
    tta = inference.predict_instances(model, x, tta=(1.0,), max_instances=512)
    r = uaps_amd.predict_tta(model, x, scales=(1.0,), want=("mask", "conf"))
    assert tta.n_maps == 2 and torch.equal(tta.labels, label_instances(r.mask, (r.conf,), max_instances=512).labels)
    assert torch.equal(tta.table[..., 7], label_instances(r.mask, (r.conf,), max_instances=512).table[..., 7])
    # a one-head model: the confidence alone
    plain = uaps_amd.net_factory("unet", 3, 4).to(DEV)
    one = inference.predict_instances(plain, x)
    assert one.n_maps == 1 and int(one.table[..., 8].abs().sum()) == 0
    assert all(r["mean0"] > 0.0 and r["mean1"] is None for rr in one.records() for r in rr)
