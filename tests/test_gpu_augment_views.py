"""-m gpu: the program-interpreting input pipeline (csrc/augment_views.hip, uaps_amd/pipelines.py) against its stage-by-stage numpy
restatement (tests/augment_views_ref.py), against the one-recipe kernel on the recipe they share, one launch of two views against
two launches, the in-kernel random draws, and the batch sources in front of the trainers.
Parity with cv2 / albumentations is UNPINNED (neither library is in the image): nothing here claims it."""
import numpy as np
import pytest
import torch

import augment_views_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_every_op_and_segment(i):
    """Every opcode, blur size, quarter turn, grid on / off and each of the three segments (tests/augment_views_ref.py::case) with
    injected noise and drop fields.  Masks and contrast means are exact.  Image values may differ from the float64 restatement only
    at rounding ties of the kernel's float32 (bilinear weights, HSV, v * f): at most CAP = 1e-3 of an image's values, by one grey
    level each.  The seeds and hand-set factors were fixed under the condition the issue sets -- the restatement in float32 against
    itself in float64 stays under a third of the cap (test_pipelines_host.py::test_case_seeds_keep_float32_ties_rare; measured: no
    value differs in any of the 24 images) -- after replacing short decimal factors (0.9, 1.15, ...), for which v * f lies ON
    an integer for a tenth of all grey levels and float32 against float64 alone differed in up to 12 % of an image."""
    from uaps_amd import pipelines as P
    c = R.case(i)
    Ho, Wo = c["out_size"]
    x, y, m = P.augment_views(_t(c["img"]), _t(c["mask"]), c["draws"], (Ho, Wo), R.MEAN, R.STD, seed=1, noise=_t(c["noise"])[None],
                              drop_u=_t(c["drop_u"])[None], return_means=True)
    assert x.shape == (1, R.B, c["img"].shape[3], Ho, Wo) and y.shape == (1, R.B, Ho, Wo) and y.dtype == torch.int64
    x, y, m = x.cpu().numpy()[0], y.cpu().numpy()[0], m.cpu().numpy()[0]
    ref = R.reference(c)
    for b, (rx, ry, rm) in enumerate(ref):
        share, worst = R.compare(x[b], rx)
        print(f"shape {i} image {b}: share of differing values {share:.2e}, largest difference {worst}, m {m[b]} / {rm}")
    for b, (rx, ry, rm) in enumerate(ref):
        assert np.array_equal(y[b], ry), f"mask {b}"
        assert m[b] == rm, f"contrast mean {b}: {m[b]} != {rm}"
        share, worst = R.compare(x[b], rx)
        assert share <= R.CAP and worst <= 1, f"image {b}: {share} of the values differ, by up to {worst}"
        # and the stored float is the normalisation of an integer grey level
        g = R.grey_levels(x[b], R.MEAN, R.STD)
        Cs = x.shape[1]
        back = (g.astype(np.float32) / np.float32(255) - np.asarray(R.MEAN[:Cs], np.float32).reshape(Cs, 1, 1)) / np.asarray(R.STD[:Cs], np.float32).reshape(Cs, 1, 1)
        assert np.abs(back - x[b]).max() < 1e-5


@pytest.mark.parametrize("Hs,Ws,Ho,Wo", [(200, 200, 64, 64), (37, 53, 32, 32)])
def test_neu_program_is_bit_identical_with_the_one_recipe_kernel(Hs, Ws, Ho, Wo):
    from uaps_amd import augment
    from uaps_amd import pipelines as P
    rng = np.random.default_rng(Hs + Wo)
    B = 12
    img = rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)
    mask = rng.integers(0, 4, (B, Hs, Ws), dtype=np.uint8)
    p = augment.draw_train_params(B, rng)
    p.ints[0, :5] = (1, 1, 1, 7, 1); p.floats[0, :3] = (1.5, 0.5, 7.0)
    p.ints[1, :5] = (0, 0, 3, 3, 0); p.floats[1, :3] = (1.0, 0.0, 0.0)
    p.ints[2, :5] = (1, 0, 2, 5, 1); p.floats[2, :3] = (1.2, 0.1, 3.3)
    p.ints[3, :5] = (0, 1, 0, 0, 1); p.floats[3, :3] = (1.37, 0.21, 5.0)
    noise = _t((rng.standard_normal((B, 3, Ho, Wo)).astype(np.float32) * p.floats[:, 2][:, None, None, None]).astype(np.float32))
    x0, y0 = augment.augment_batch(_t(img), _t(mask), p, (Ho, Wo), noise=noise)
    x1, y1 = P.augment_views(_t(img), _t(mask), P.ViewDraws(R.neu_rows(p), None, None), (Ho, Wo), noise=noise[None])
    assert torch.equal(x1[0], x0) and torch.equal(y1[0], y0)


def test_two_views_in_one_launch_equal_two_launches_and_the_empty_program_is_the_identity():
    from uaps_amd import augment
    from uaps_amd import pipelines as P
    rng = np.random.default_rng(21)
    B, Hs, Ws, Ho, Wo = 5, 45, 61, 40, 40                                     # 1600 pixels: 6.25 / 12.5 workgroups per image
    img, mask = _t(rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)), _t(rng.integers(0, 4, (B, Hs, Ws), dtype=np.uint8))
    weak, strong = P.draw("ucc_weak", B, rng, (Ho, Wo)), P.draw("ucc_strong", B, rng, (Ho, Wo))
    P.set_program(strong.rows[0], [("blur", 5), ("hue", 0.11), ("contrast", 1.13), ("pixdrop", 0.02), ("noise", 6.0)])
    P.set_program(weak.rows[1], [("bc", 1.31, 0.12), ("blur", 3), ("noise", 4.0)])
    strong.rows[2]["hflip"] = 1                                              # the views' geometry may differ as well
    noise = _t(rng.standard_normal((2, B, 3, Ho, Wo)).astype(np.float32) * 5)
    drop = _t(rng.random((2, B, Ho, Wo), dtype=np.float32))
    x2, y2, m2 = P.augment_views(img, mask, [weak, strong], (Ho, Wo), noise=noise, drop_u=drop, return_means=True)
    xa, ya, ma = P.augment_views(img, mask, weak, (Ho, Wo), noise=noise[:1], drop_u=drop[:1], return_means=True)
    xb, yb, mb = P.augment_views(img, mask, strong, (Ho, Wo), noise=noise[1:], drop_u=drop[1:], return_means=True)
    assert torch.equal(x2[0], xa[0]) and torch.equal(x2[1], xb[0]) and torch.equal(y2[0], ya[0]) and torch.equal(y2[1], yb[0])
    assert torch.equal(m2[0], ma[0]) and torch.equal(m2[1], mb[0]) and float(m2[1, 0]) >= 0 and float(m2[0, 0]) == -1
    # resize_only + nothing: the identity_params of the one-recipe path
    ident = P.draw("resize_only", B, rng)
    xi, yi = P.augment_views(img, mask, [ident, strong], (Ho, Wo), noise=noise, drop_u=drop)
    x0, y0 = augment.augment_batch(img, mask, augment.identity_params(B), (Ho, Wo))
    assert torch.equal(xi[0], x0) and torch.equal(yi[0], y0) and torch.equal(xi[1], x2[1])
    xn, yn = P.augment_views(img, None, ident, (Ho, Wo))
    assert yn is None and torch.equal(xn[0], x0)


def test_in_kernel_draws():
    """Philox paths on a mid-grey 64 x 64 image: the noise bounds of test_gpu_augment.py (mean -0.5 +- 0.15 from the truncation,
    sigma within 5 %), the dropped share within 4 sigma of p = 0.01 over 4 * 64 * 64 pixels, seeds reproduce / differ."""
    from uaps_amd import pipelines as P
    B = 4
    img = _t(np.full((B, 64, 64, 3), 128, np.uint8))
    mean, std = np.asarray(R.MEAN, np.float32)[None, :, None, None], np.asarray(R.STD, np.float32)[None, :, None, None]
    rows = P.empty_rows(B)
    for r in rows:
        P.set_program(r, [("noise", 6.0)])
    d = P.ViewDraws(rows, None, None)
    x, _ = P.augment_views(img, None, d, (64, 64), seed=1234)
    g = (x[0].cpu().numpy() * std + mean) * 255.0 - 128.0
    print("noise mean", g.mean(), "std", g.std())
    assert abs(g.mean() + 0.5) < 0.15 and abs(g.std() - 6.0) < 0.3
    assert np.abs(np.corrcoef(g[:, 0].ravel(), g[:, 1].ravel())[0, 1]) < 0.05      # the channels draw separately
    x2, _ = P.augment_views(img, None, d, (64, 64), seed=1234)
    x3, _ = P.augment_views(img, None, d, (64, 64), seed=1235)
    assert torch.equal(x, x2) and not torch.equal(x, x3)
    p = 0.01
    for r in rows:
        P.set_program(r, [("pixdrop", p)])
    xd, _ = P.augment_views(img, None, d, (64, 64), seed=77)
    gd = np.rint((xd[0].cpu().numpy() * std + mean) * 255.0)
    assert set(np.unique(gd)) <= {0.0, 128.0}
    dropped = gd[:, 0] == 0
    assert (dropped == (gd[:, 1] == 0)).all() and (dropped == (gd[:, 2] == 0)).all()   # one draw per pixel, all channels
    n = dropped.size
    print("dropped share", dropped.mean())
    assert abs(dropped.mean() - p) <= 4 * np.sqrt(p * (1 - p) / n)
    xd2, _ = P.augment_views(img, None, d, (64, 64), seed=77)
    xd3, _ = P.augment_views(img, None, d, (64, 64), seed=78)
    assert torch.equal(xd, xd2) and not torch.equal(xd, xd3)
    # two views of one launch draw different fields from one seed
    xv, _ = P.augment_views(img, None, [d, d], (64, 64), seed=77)
    assert torch.equal(xv[0], xd[0]) and not torch.equal(xv[1], xv[0])


def test_ucc_array_batches_feed_the_ucc_trainer():
    import uaps_amd
    rng = np.random.default_rng(8)
    lab_i, lab_m = rng.integers(0, 256, (4, 50, 70, 3), dtype=np.uint8), rng.integers(0, 4, (4, 50, 70), dtype=np.uint8)
    unl_i, unl_m = rng.integers(0, 256, (6, 50, 70, 3), dtype=np.uint8), rng.integers(0, 4, (6, 50, 70), dtype=np.uint8)
    src = uaps_amd.UCCArrayBatches(lab_i, lab_m, unl_i, unl_m, 2, seed=3, out_size=(64, 64), device=DEV)
    assert len(src.train) == 2 and len(src.unlabeled) == 3
    item = next(iter(src.unlabeled))
    assert len(item) == 4 and item[0].shape == item[1].shape == (2, 3, 64, 64) and item[2].dtype == torch.int64
    assert torch.equal(item[2], item[3])                                      # neither view moves the mask
    torch.manual_seed(5)
    tr = uaps_amd.UCCTrainer(uaps_amd.net_factory("unet_ucc", 3, 4).to(DEV))
    val = list(uaps_amd.ArrayBatches(lab_i, lab_m, "resize_only", 2, out_size=(64, 64), shuffle=False, device=DEV))
    hist = tr.fit(src.train, src.unlabeled, val, epochs=2, iter_per_epoch=3)
    assert len(hist) == 1 and tr.iter_num == 2
    for k in ("loss", "ce", "dice", "ps", "sup", "unsup", "val_mdice", "val_ce"):
        assert np.isfinite(hist[0][k]), k


def test_one_channel_array_batches_feed_the_baseline_trainer():
    import uaps_amd
    rng = np.random.default_rng(9)
    img, mask = rng.integers(0, 256, (4, 60, 60), dtype=np.uint8), rng.integers(0, 7, (4, 60, 60), dtype=np.uint8)
    src = uaps_amd.ArrayBatches(img, mask, "dagm_labelled", 2, out_size=(64, 64), device=DEV)
    assert src.mean == (0.5314,) and src.std == (0.1357,)
    x, y = next(iter(src))
    assert x.shape == (2, 1, 64, 64) and y.shape == (2, 64, 64) and int(y.max()) < 7
    torch.manual_seed(6)
    tr = uaps_amd.BaselineTrainer(uaps_amd.net_factory("unet", 1, 7).to(DEV))
    out = tr.train_step(x, y)
    assert torch.isfinite(out["loss"]).item()
